"""Per-validator bond summary per epoch, host side (no GPU): the C-ABI of
yuma_run_rowstat and its companions, the yuma_rowstat_native truth table, the
refusals that come back before the first launch (equal from the direct run and
the graph form, in the order the header documents), the workspace arithmetic,
the register report of the RS kernels, engine.settled_epoch_rows on hand-made
arrays, and the want_row_stats argument checks of engine.run, which raise
before anything touches a device."""

from __future__ import annotations

import ctypes
import os
import re

import pytest
import torch

from yuma_simulation._internal import engine
from yuma_simulation._internal.cases import cases as builtin_cases
from yuma_simulation._internal.simulation_utils import SimulationRun, run_simulations
from yuma_simulation._internal.yumas import YumaConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("yuma_run_rowstat", "yuma_graph_create_rowstat", "yuma_rowstat_native", "yuma_workspace_bytes_rowstat")
RUST, Y1, Y2, Y3, Y4 = range(5)
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4
MAXV = engine.MAX_VALIDATORS


def header_code():
    text = open(os.path.join(ROOT, "include", "yuma_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def proto(name):
    return re.search(r"\b(\w+)\s+" + name + r"\s*\((.*?)\)\s*;", header_code(), flags=re.S)


def test_header_declares_the_entry_points():
    for name in NEW_FUNCTIONS[:3]:
        assert proto(name).group(1) == "int", name
    assert proto("yuma_workspace_bytes_rowstat").group(1) == "size_t"
    for name in NEW_FUNCTIONS[:2]:
        args = re.sub(r"\s+", " ", proto(name).group(2))
        # yuma_run_rows's arguments with B_rowstat after B_rows
        assert "const int32_t* rows_dev, int n_rows, float* B_rows, float* B_rowstat, void* workspace" in args
        rows = re.sub(r"\s+", " ", proto(name.replace("rowstat", "rows")).group(2))
        assert args.replace("float* B_rowstat, ", "") == rows
    args = [re.sub(r"\s+", " ", a).strip() for a in proto("yuma_rowstat_native").group(2).split(",")]
    assert args == ["int variant", "int N", "int E", "int V", "int M", "const yuma_outputs_t* out", "int flags"]


def test_library_exports_and_argtypes_match_the_header():
    lib = engine.load_library()
    for name in NEW_FUNCTIONS:
        assert name in engine.EXPORTED_SYMBOLS, name
        fn = getattr(lib, name)
        n_params = len([a for a in proto(name).group(2).split(",") if a.strip()])
        assert len(fn.argtypes) == n_params, name
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    a, b = list(lib.yuma_run_rows.argtypes), list(lib.yuma_run_rowstat.argtypes)
    assert b == a[:20] + [vp] + a[20:]
    a, b = list(lib.yuma_graph_create_rows.argtypes), list(lib.yuma_graph_create_rowstat.argtypes)
    assert b == a[:21] + [vp] + a[21:]
    assert list(lib.yuma_rowstat_native.argtypes) == [i32] * 5 + [vp, i32]
    assert list(lib.yuma_workspace_bytes_rowstat.argtypes) == [i32] * 6
    assert lib.yuma_workspace_bytes_rowstat.restype is ctypes.c_size_t
    # the records the issue leaves alone
    assert ctypes.sizeof(engine.YumaScanPlanC) == 80 and ctypes.sizeof(engine.YumaRunOptionsC) == 32


@pytest.mark.parametrize("V,M", [(5, 8), (67, 12), (MAXV, 8), (9, 520)])
def test_rowstat_native_truth_table(V, M):
    N, E = 2, 6
    for variant in (Y3, Y4):
        assert engine.rowstat_native(variant, N, E, V, M)
        assert engine.rowstat_native(variant, N, E, V, M, want=("D", "R", "P", "T", "Sn", "bond_alpha", "alpha_ab"))
        assert not engine.rowstat_native(variant, N, E, V, 10)             # the scalar form
        assert not engine.rowstat_native(variant, N, E, V, M, shared_inputs=True)
        assert not engine.rowstat_native(variant, N, E, V, M, w_u16=True)
        assert not engine.rowstat_native(variant, N, E, V, M, True)        # a history in the same run
        for name in ("Wn", "Wc", "Wb", "B_inst", "Tv"):
            assert not engine.rowstat_native(variant, N, E, V, M, want=(name,)), name
        assert not engine.rowstat_native(variant, N, E, MAXV + 1, M)
        assert not engine.rowstat_native(variant, 0, E, V, M) and not engine.rowstat_native(variant, N, 0, V, M)
    for variant in (RUST, Y1, Y2):
        assert not engine.rowstat_native(variant, N, E, V, M)
    assert not engine.rowstat_native(7, N, E, V, M)


def test_rowstat_native_cases_reach_the_flat_scans():
    """The native set is the calls plan_scan sends to the flat history-less shapes."""
    for variant in (Y3, Y4):
        for N, V, M in ((2, 5, 260), (64, 512, 8), (1, 1030, 8), (2, 9, 520), (1, MAXV, 8)):
            assert engine.rowstat_native(variant, N, 6, V, M)
            plan = engine.scan_plan(variant, N, 6, V, M)
            assert plan.form == "k_bonds_elem" and plan.shape in ("flat1", "flat2") and plan.vector_form, plan
            assert plan.rq and not plan.hist and plan.dpl == "QTE", plan


@pytest.mark.parametrize("variant,N,E,V,M", [(Y3, 2, 6, 5, 260), (Y4, 64, 4, 512, 8), (Y4, 1, 19, 9, 520),
                                             (Y1, 2, 6, 5, 8), (Y3, 1, 1, 1, 4)])
def test_workspace_bytes_rowstat(variant, N, E, V, M):
    lib = engine.load_library()
    for full in (0, 1):
        base = int(lib.yuma_workspace_bytes(variant, N, E, V, M, full))
        got = engine.workspace_bytes_rowstat(variant, N, E, V, M, bool(full))
        # the run's own workspace on its 256-byte granule, and one padded DP_QTE array of quad partials:
        # [N][ceil(tiles / 4)][V][E rounded up to 16] floats
        quads = ((M + 63) // 64 + 3) // 4
        part = (N * quads * V * ((E + 15) // 16 * 16) * 4 + 255) // 256 * 256
        assert got == (base + 255) // 256 * 256 + part and got >= base
    assert engine.workspace_bytes_rowstat(variant, 0, E, V, M) == 0


# ---------------------------------------------------------------------------
# refusals before the first launch: no GPU, no HIP call. The pointers are never
# dereferenced (any non-null value stands for device memory).
# ---------------------------------------------------------------------------
P = 0x1000  # a non-null "device pointer"


def call_both(variant=Y3, N=2, E=6, K=0, V=5, M=8, sched=None, watch=None, n_watch=0, b_watch=None, b_move=None,
              rows=None, n_rows=0, b_rows=None, b_rowstat=P, ws_bytes=None, flags=0, hist=None, W=P, want=()):
    """(code, text) of yuma_run_rowstat and of yuma_graph_create_rowstat."""
    lib = engine.load_library()
    outs = engine.YumaOutputsC(Dn=P, C=P, I=P, B_final=P, B_hist=hist, **{k: P for k in want})
    opts = engine.YumaRunOptionsC(flags=flags, hist_stride=1, hist_first=0)
    if ws_bytes is None:
        ws_bytes = 1 << 40
    common = (variant, P, N, E, K, V, M, W, P, sched, None, None, ctypes.addressof(outs), watch, n_watch, b_watch,
              b_move, rows, n_rows, b_rows, b_rowstat, P, ws_bytes, 0, ctypes.addressof(opts))
    rc_run = lib.yuma_run_rowstat(*common, None, None)
    msg_run = lib.yuma_last_error().decode()
    h = ctypes.c_void_p()
    rc_graph = lib.yuma_graph_create_rowstat(ctypes.byref(h), *common)
    msg_graph = lib.yuma_last_error().decode()
    assert h.value is None
    return (rc_run, msg_run), (rc_graph, msg_graph)


WATCH = dict(watch=P, n_watch=3, b_watch=P)
ROWS = dict(rows=P, n_rows=2, b_rows=P)


@pytest.mark.parametrize("kw,code,text", [
    (dict(N=0), EINVAL, "sizes must be positive"),
    (dict(V=MAXV + 1), EUNSUPPORTED, "YUMA_MAX_VALIDATORS"),
    (dict(W=None), EINVAL, "null params"),
    (dict(sched=P, K=0), EINVAL, "K=0"),
    (dict(sched=None, K=3), EINVAL, "K=3"),
    # the optional lists: given in part, their own checks
    (dict(n_watch=3), EINVAL, "watch list or B_watch is NULL"),
    (dict(rows=P, n_rows=0, b_rows=P), EINVAL, "n_rows=0"),
    (dict(n_rows=2), EINVAL, "row list or B_rows is NULL"),
    # B_rowstat: after the lists' checks, before the workspace size and before "not native"
    (dict(b_rowstat=None), EINVAL, "B_rowstat is NULL"),
    (dict(b_rowstat=None, n_rows=2), EINVAL, "row list or B_rows is NULL"),
    (dict(b_rowstat=None, ws_bytes=16), EINVAL, "B_rowstat is NULL"),
    (dict(b_rowstat=None, variant=Y1), EINVAL, "B_rowstat is NULL"),
    (dict(b_rowstat=None, sched=P, K=2), EINVAL, "B_rowstat is NULL"),
    # no lists at all is accepted up to the workspace check, which comes before "not native"
    (dict(ws_bytes=16), EWORKSPACE, "workspace"),
    (dict(ws_bytes=16, **WATCH, **ROWS), EWORKSPACE, "workspace"),
    (dict(ws_bytes=16, variant=Y1), EWORKSPACE, "workspace"),
    # the lists' native refusals come first ...
    (dict(variant=Y1, **WATCH), EUNSUPPORTED, "yuma_watch_native"),
    (dict(variant=Y1, **ROWS), EUNSUPPORTED, "yuma_rows_native"),
    # ... then what the summary does not combine with: a schedule, a B_move
    (dict(sched=P, K=2), EUNSUPPORTED, "does not combine"),
    (dict(b_move=P), EUNSUPPORTED, "does not combine"),
    (dict(sched=P, K=2, M=10), EUNSUPPORTED, "yuma_sched_native"),   # (the schedule's own refusal is earlier still)
    # ... then the predicate
    (dict(variant=RUST), EUNSUPPORTED, "yuma_rowstat_native"),
    (dict(variant=Y1), EUNSUPPORTED, "yuma_rowstat_native"),
    (dict(variant=Y2), EUNSUPPORTED, "yuma_rowstat_native"),
    (dict(M=10), EUNSUPPORTED, "yuma_rowstat_native"),
    (dict(M=10, **WATCH, **ROWS), EUNSUPPORTED, "yuma_rowstat_native"),  # the list kernels take any M; the summary does not
    (dict(flags=engine.RUN_SHARED_INPUTS), EUNSUPPORTED, "yuma_rowstat_native"),
    (dict(hist=P), EUNSUPPORTED, "yuma_rowstat_native"),
    (dict(want=("Wn",)), EUNSUPPORTED, "yuma_rowstat_native"),
    (dict(want=("Tv",)), EUNSUPPORTED, "yuma_rowstat_native"),
    # ... then the vector form
    (dict(W=P + 4), EUNSUPPORTED, "needs the vector form"),
    (dict(W=P + 4, **WATCH), EUNSUPPORTED, "needs the vector form"),
    # ... all before YUMA_RUN_HIST_BF16 / YUMA_RUN_W_U16
    (dict(flags=engine.RUN_HIST_BF16), EUNSUPPORTED, "yuma_rowstat_native"),
    (dict(flags=engine.RUN_W_U16), EUNSUPPORTED, "yuma_rowstat_native"),
])
def test_refusals_without_a_gpu_are_equal_from_run_and_graph(kw, code, text):
    run, graph = call_both(**kw)
    assert run[0] == code and text in run[1], run
    assert graph == run


def test_the_exact_workspace_passes_the_size_check():
    """One byte short is the workspace refusal; the exact size reaches the next one (W off its alignment)."""
    need = engine.workspace_bytes_rowstat(Y3, 2, 6, 5, 8)
    assert call_both(ws_bytes=need - 1, W=P + 4)[0][0] == EWORKSPACE
    run, _ = call_both(ws_bytes=need, W=P + 4)
    assert run[0] == EUNSUPPORTED and "vector form" in run[1]
    # the plain run's workspace is too small
    assert call_both(ws_bytes=engine.workspace_bytes(Y3, 2, 6, 5, 8, False), W=P + 4)[0][0] == EWORKSPACE


def test_run_rows_still_refuses_an_empty_row_list():
    lib = engine.load_library()
    outs = engine.YumaOutputsC(Dn=P, C=P, I=P, B_final=P)
    opts = engine.YumaRunOptionsC(flags=0, hist_stride=1, hist_first=0)
    rc = lib.yuma_run_rows(Y3, P, 2, 6, 0, 5, 8, P, P, None, None, None, ctypes.addressof(outs), None, 0, None, None,
                           None, 0, None, P, 1 << 40, 0, ctypes.addressof(opts), None, None)
    assert rc == EINVAL and "n_rows=0" in lib.yuma_last_error().decode()


def test_graph_handle_is_checked_after_the_options():
    lib = engine.load_library()
    outs = engine.YumaOutputsC(Dn=P, C=P, I=P, B_final=P)
    bad = engine.YumaRunOptionsC(flags=0, hist_stride=-1)
    args = (Y3, P, 2, 6, 0, 5, 8, P, P, None, None, None, ctypes.addressof(outs), None, 0, None, None, None, 0, None,
            P, P, 1 << 40, 0)
    assert lib.yuma_graph_create_rowstat(None, *args, ctypes.addressof(bad)) == EINVAL
    assert "hist_stride" in lib.yuma_last_error().decode()
    ok = engine.YumaRunOptionsC()
    assert lib.yuma_graph_create_rowstat(None, *args, ctypes.addressof(ok)) == EINVAL
    assert "graph handle" in lib.yuma_last_error().decode()


def test_scan_plan_record_is_untouched():
    names = [n for n, _ in engine.YumaScanPlanC._fields_]
    assert "rs" not in names and len(names) == 19


# ---------------------------------------------------------------------------
# the register report of the RS kernels, from the built library's code object
# ---------------------------------------------------------------------------
def test_no_rs_kernel_spills_or_uses_scratch():
    """The 4 row-summary forms of k_bonds_elem (Yuma 3 / Yuma 4 on the one-row and
    the two-row flat shape) report no spilled VGPR, no spilled SGPR and no
    scratch, and take BondArgs' block with the two pointers appended."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kcompare

    meta = kcompare.kernels(engine.LIB_PATH)
    forms = kcompare.elem_forms(meta, "RS")
    rs = {k: meta[k][2] for k in forms}
    assert len(rs) == 4, sorted(rs)
    shapes = {(variant, re.match(r"Li(\d)E", shape).group(1)) for variant, shape, _ in forms.values()}
    assert shapes == {("3", "1"), ("3", "2"), ("4", "1"), ("4", "2")}
    fields = dict(zip(kcompare.FIELDS, range(len(kcompare.FIELDS))))
    for name, m in rs.items():
        for f in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
            assert m[fields[f]] == "0", (name, f, m)
        assert m[fields["kernarg_segment_size"]] == "232", (name, m)   # BondArgs' 216 bytes and the two pointers


# ---------------------------------------------------------------------------
# engine.settled_epoch_rows and the dense reduction: pure torch, on CPU tensors
# ---------------------------------------------------------------------------
def rs3(moved, size=None, total=None):
    moved = torch.tensor(moved, dtype=torch.float32)
    size = torch.ones_like(moved) if size is None else torch.tensor(size, dtype=torch.float32)
    total = torch.zeros_like(moved) if total is None else torch.tensor(total, dtype=torch.float32)
    return torch.stack([moved, size, total], dim=-1)


def test_settled_epoch_rows_on_hand_made_arrays():
    nan = float("nan")
    # [E = 4, N = 1, V = 3]: settles at 0; never settles; a NaN in the tail
    m = rs3([[[0.0, 1.0, 1.0]], [[0.0, 1.0, 0.0]], [[0.0, 1.0, 0.0]], [[0.0, 1.0, nan]]])
    r = engine.settled_epoch_rows(m, 0.1)
    assert r.dtype == torch.int64 and r.shape == (1, 3) and r.tolist() == [[0, 4, 4]]
    # [E = 3, N = 2, V = 2] with different answers per scenario and validator; <= tol counts
    m = rs3([[[1.0, 0.5], [0.0, 1.0]], [[0.1, 0.0], [0.0, 0.2]], [[0.0, 0.0], [0.0, 0.0]]])
    assert engine.settled_epoch_rows(m, 0.1).tolist() == [[1, 1], [0, 2]]
    assert engine.settled_epoch_rows(m.numpy(), 0.1).tolist() == [[1, 1], [0, 2]]
    # one scenario's [E, V, 3]
    assert engine.settled_epoch_rows(m[:, 1], 0.1).tolist() == [0, 2]
    # relative: Yuma 3's 2^64 scale, per validator; the total column plays no part
    big = 2.0 ** 64
    m = rs3([[[big, big]], [[big * 1e-3, big * 1e-7]], [[big * 1e-7, big * 1e-8]]], [[[big, big]]] * 3,
            [[[nan, 5.0]]] * 3)
    assert engine.settled_epoch_rows(m, 1e-6).tolist() == [[3, 3]]
    assert engine.settled_epoch_rows(m, 1e-6, relative=True).tolist() == [[2, 1]]
    # it is settled_epoch of the first two columns
    assert torch.equal(engine.settled_epoch_rows(m, 1e-6, relative=True), engine.settled_epoch(m[..., :2], 1e-6, relative=True))
    assert engine.settled_epoch_rows(torch.zeros((0, 2, 3, 3)), 0.1).tolist() == [[0, 0, 0], [0, 0, 0]]
    for bad in (torch.zeros((3, 2, 2)), torch.zeros((3, 3))):
        with pytest.raises(ValueError, match="B_rowstat"):
            engine.settled_epoch_rows(bad, 0.1)


def test_rowstat_from_history_is_the_definition():
    g = torch.Generator().manual_seed(3)
    hist = torch.rand((5, 2, 3, 4), generator=g) - 0.5
    b0 = torch.rand((2, 3, 4), generator=g)
    for init in (None, b0):
        full = torch.cat([torch.zeros_like(hist[:1]) if init is None else init[None], hist])
        got = engine.rowstat_from_history(hist, init)
        assert got.shape == (5, 2, 3, 3) and got.dtype == torch.float32
        assert torch.equal(got[..., 0], (full[1:] - full[:-1]).abs().amax(-1))
        assert torch.equal(got[..., 1], hist.abs().amax(-1))
        assert torch.equal(got[..., 2], hist.sum(-1))
        # amax over v is the movement
        assert torch.equal(got[..., :2].amax(2), engine.move_from_history(hist, init))


# ---------------------------------------------------------------------------
# engine.run validates want_row_stats on the host
# ---------------------------------------------------------------------------
@pytest.fixture()
def no_device(monkeypatch):
    """Any request for the device fails the test: validation comes first."""
    def boom():
        raise AssertionError("a device was asked for before want_row_stats was validated")
    monkeypatch.setattr(engine, "device", boom)


def run_args(E=3, N=2, V=5, M=8):
    g = torch.Generator().manual_seed(1)
    W, S = torch.rand((E, N, V, M), generator=g), torch.rand((E, N, V), generator=g) + 0.5
    return Y3, [engine.make_params(Y3, YumaConfig())] * N, W, S


def test_run_rejects_bad_want_row_stats_arguments_before_touching_the_device(no_device):
    variant, params, W, S = run_args()
    for bad in (1, "yes", None, [True]):
        with pytest.raises(ValueError, match="want_row_stats"):
            engine.run(variant, params, W, S, want_row_stats=bad)
    with pytest.raises(ValueError, match="want_row_stats"):
        engine.run(variant, params, W[:1], S[:1], want_row_stats=True, single_call=True)
    with pytest.raises(ValueError, match="want_row_stats"):
        engine.RunGraph(variant, params, W, S, want_row_stats=1)


@pytest.mark.parametrize("kw,text", [
    (dict(resets=[(1, 0, 2, engine.RESET_ALWAYS)]), "resets= does not combine with want_row_stats"),
    (dict(row_resets=[(1, 0, 2)]), "row_resets= does not combine with want_row_stats"),
])
def test_run_rejects_the_event_lists_before_touching_the_device(no_device, kw, text):
    """resets= and row_resets= do not combine with want_row_stats at all (ValueError). sched= and want_move do: the
    C entry points refuse them beside the summary (the refusal table above) and run reduces a dense history
    (tests/test_gpu_rowstat.py)."""
    variant, params, W, S = run_args()
    with pytest.raises(ValueError, match=text):
        engine.run(variant, params, W, S, want_row_stats=True, **kw)
    with pytest.raises(ValueError, match=text):
        engine.RunGraph(variant, params, W, S, want_row_stats=True, **kw)


def test_run_simulations_rejects_the_event_lists_before_touching_the_device(no_device):
    case = builtin_cases[0]
    runs = [SimulationRun(case, "Yuma 3 (Rhef)", YumaConfig())]
    with pytest.raises(ValueError, match="bonds_row_stats does not combine"):
        run_simulations(runs, bonds_row_stats=True, bond_resets=[[(1, 0)]])
    with pytest.raises(ValueError, match="bonds_row_stats does not combine"):
        run_simulations(runs, bonds_row_stats=True, validator_resets=[[(1, 0)]])


def test_run_result_has_the_new_field_with_a_default():
    r = engine.RunResult(None, None, None, None, None, {})
    assert r.B_rowstat is None
