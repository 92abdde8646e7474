"""Watched validator rows, host side (no GPU): the C-ABI of yuma_run_rows and
its companions, the yuma_rows_native truth table, the refusals that come back
before the first launch (equal from the direct run and the graph form, in the
order the header documents; a NULL B_move is no refusal here), the argument
checks of engine.run(watch_rows=) and run_simulations(bonds_validators=), which
raise before anything touches a device, and the register report of the
k_bonds_rows instantiations."""

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
NEW_FUNCTIONS = ("yuma_run_rows", "yuma_graph_create_rows", "yuma_rows_native")
RUST, Y1, Y2, Y3, Y4 = range(5)
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4
MAXV = engine.MAX_VALIDATORS


def header_code():
    text = open(os.path.join(ROOT, "include", "yuma_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def proto(name):
    return re.search(r"\b(\w+)\s+" + name + r"\s*\((.*?)\)\s*;", header_code(), flags=re.S)


def test_header_declares_the_three_entry_points():
    for name in NEW_FUNCTIONS:
        assert proto(name).group(1) == "int", name
    rows = "const int32_t* rows_dev, int n_rows, float* B_rows, "
    for name in NEW_FUNCTIONS[:2]:
        args = re.sub(r"\s+", " ", proto(name).group(2))
        # yuma_run_move's arguments with the row list, its length and B_rows after B_move
        assert "float* B_move, " + rows + "void* workspace" in args
        move = re.sub(r"\s+", " ", proto(name.replace("rows", "move")).group(2))
        assert args.replace(rows, "") == move
    args = [re.sub(r"\s+", " ", a).strip() for a in proto("yuma_rows_native").group(2).split(",")]
    assert args == ["int variant", "int N", "int E", "int V", "int M", "int n_rows", "int flags"]


def test_library_exports_and_argtypes_match_the_header():
    lib = engine.load_library()
    for name in NEW_FUNCTIONS:
        assert name in engine.EXPORTED_SYMBOLS, name
        fn = getattr(lib, name)
        n_params = len([a for a in proto(name).group(2).split(",") if a.strip()])
        assert len(fn.argtypes) == n_params, name
        assert fn.restype is ctypes.c_int
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    a, b = list(lib.yuma_run_move.argtypes), list(lib.yuma_run_rows.argtypes)
    assert b == a[:17] + [vp, i32, vp] + a[17:]
    a, b = list(lib.yuma_graph_create_move.argtypes), list(lib.yuma_graph_create_rows.argtypes)
    assert b == a[:18] + [vp, i32, vp] + a[18:]
    assert list(lib.yuma_rows_native.argtypes) == [i32] * 7


@pytest.mark.parametrize("M", [6, 8])
@pytest.mark.parametrize("V", [5, 1030])
def test_rows_native_truth_table(V, M):
    N, E, nr = 2, 6, 3
    for variant in (Y3, Y4):
        assert engine.rows_native(variant, N, E, V, M, nr)
    for variant in (RUST, Y1, Y2):
        assert not engine.rows_native(variant, N, E, V, M, nr)
    assert not engine.rows_native(Y3, N, E, V, M, nr, shared_inputs=True)
    # uint16 weights: exactly where the run reads them natively
    for variant in (Y3, Y4):
        assert engine.rows_native(variant, N, E, V, M, nr, w_u16=True) == engine.u16_native(variant, N, E, V, M)
    assert engine.u16_native(Y3, N, E, 5, 8) and not engine.u16_native(Y3, N, E, 5, 6)
    assert not engine.u16_native(Y3, N, E, 1030, 8)
    # sizes
    assert not engine.rows_native(Y3, N, E, V, M, 0)
    assert engine.rows_native(Y3, N, E, MAXV, M, nr) and not engine.rows_native(Y3, N, E, MAXV + 1, M, nr)
    lib = engine.load_library()
    assert lib.yuma_rows_native(Y3, N, E, V, M, nr, 0) == 1 and lib.yuma_rows_native(Y1, N, E, V, M, nr, 0) == 0


# ---------------------------------------------------------------------------
# refusals before the first launch: no GPU, no HIP call. The pointers are never
# dereferenced (any non-null value stands for device memory).
# ---------------------------------------------------------------------------
P = 0x1000  # a non-null "device pointer"


def call_both(variant=Y3, N=2, E=6, K=0, V=5, M=8, sched=None, watch=None, n_watch=0, b_watch=None, b_move=None,
              rows=P, n_rows=3, b_rows=P, ws_bytes=None, flags=0, hist=None, W=P, want=(), stride=1):
    """(code, text) of yuma_run_rows and of yuma_graph_create_rows."""
    lib = engine.load_library()
    outs = engine.YumaOutputsC(Dn=P, C=P, I=P, B_final=P, B_hist=hist, **{k: P for k in want})
    opts = engine.YumaRunOptionsC(flags=flags, hist_stride=stride, hist_first=0)
    if ws_bytes is None:
        ws_bytes = 1 << 40
    common = (variant, P, N, E, K, V, M, W, P, sched, None, None, ctypes.addressof(outs), watch, n_watch, b_watch,
              b_move, rows, n_rows, b_rows, P, ws_bytes, 0, ctypes.addressof(opts))
    rc_run = lib.yuma_run_rows(*common, None, None)
    msg_run = lib.yuma_last_error().decode()
    h = ctypes.c_void_p()
    rc_graph = lib.yuma_graph_create_rows(ctypes.byref(h), *common)
    msg_graph = lib.yuma_last_error().decode()
    assert h.value is None
    return (rc_run, msg_run), (rc_graph, msg_graph)


WATCH = dict(watch=P, n_watch=3, b_watch=P)


@pytest.mark.parametrize("kw,code,text", [
    # the options
    (dict(flags=64), EINVAL, "unknown run flags"),
    (dict(stride=-1, N=0), EINVAL, "hist_stride"),
    # sizes, NULL pointers, the schedule's pair
    (dict(N=0, W=None), EINVAL, "sizes must be positive"),
    (dict(V=MAXV + 1, W=None), EUNSUPPORTED, "YUMA_MAX_VALIDATORS"),
    (dict(W=None, n_rows=0), EINVAL, "null params"),
    (dict(sched=P, K=0, n_rows=0), EINVAL, "K=0"),
    (dict(sched=None, K=3, rows=None), EINVAL, "K=3"),
    # the column list's checks, before the row list's
    (dict(watch=P, n_watch=0, b_watch=P, n_rows=0), EINVAL, "n_watch=0"),
    (dict(n_watch=-2, n_rows=0), EINVAL, "n_watch=-2"),
    (dict(n_watch=3, rows=None), EINVAL, "watch list or B_watch is NULL"),
    # a NULL B_move is "no movement output": the next refusal in line answers, never "B_move is NULL"
    (dict(b_move=None, n_rows=0), EINVAL, "n_rows=0"),
    (dict(b_move=None, ws_bytes=16), EWORKSPACE, "workspace"),
    (dict(b_move=None, variant=Y1), EUNSUPPORTED, "yuma_rows_native"),
    # n_rows < 1, then a NULL list or B_rows; all before the workspace size
    (dict(n_rows=0), EINVAL, "n_rows=0"),
    (dict(n_rows=-1, rows=None, ws_bytes=16), EINVAL, "n_rows=-1"),
    (dict(rows=None), EINVAL, "row list or B_rows is NULL"),
    (dict(b_rows=None, ws_bytes=16), EINVAL, "row list or B_rows is NULL"),
    (dict(rows=None, variant=Y1, **WATCH), EINVAL, "row list or B_rows is NULL"),
    (dict(n_rows=1 << 20, N=1 << 10, M=1 << 12), EINVAL, "row kernel's grid"),
    # the workspace size, before every "not native"
    (dict(ws_bytes=16), EWORKSPACE, "workspace"),
    (dict(ws_bytes=16, variant=Y1, **WATCH), EWORKSPACE, "workspace"),
    (dict(ws_bytes=16, flags=engine.RUN_SHARED_INPUTS, b_move=P), EWORKSPACE, "workspace"),
    # schedule, column list, movement (only with a B_move), rows
    (dict(sched=P, K=3, M=10), EUNSUPPORTED, "yuma_sched_native"),
    (dict(sched=P, K=3, variant=Y1, b_move=P, **WATCH), EUNSUPPORTED, "yuma_sched_native"),
    (dict(variant=Y1, b_move=P, **WATCH), EUNSUPPORTED, "yuma_watch_native"),
    (dict(flags=engine.RUN_SHARED_INPUTS, **WATCH), EUNSUPPORTED, "yuma_watch_native"),
    (dict(variant=Y1, b_move=P), EUNSUPPORTED, "yuma_move_native"),
    (dict(M=10, b_move=P), EUNSUPPORTED, "yuma_move_native"),
    (dict(hist=P, b_move=P), EUNSUPPORTED, "yuma_move_native"),
    (dict(W=P + 4, b_move=P), EUNSUPPORTED, "needs the vector form"),
    (dict(variant=RUST), EUNSUPPORTED, "yuma_rows_native"),
    (dict(variant=Y1), EUNSUPPORTED, "yuma_rows_native"),
    (dict(variant=Y2, M=10), EUNSUPPORTED, "yuma_rows_native"),
    (dict(flags=engine.RUN_SHARED_INPUTS), EUNSUPPORTED, "yuma_rows_native"),
    # ... then the flags, as ever
    (dict(flags=engine.RUN_HIST_BF16), EINVAL, "without out->B_hist"),
    (dict(flags=engine.RUN_HIST_BF16, hist=P, M=10), EUNSUPPORTED, "yuma_hist_bf16_native"),
    (dict(flags=engine.RUN_W_U16, M=10), EUNSUPPORTED, "yuma_u16_native"),
    (dict(flags=engine.RUN_W_U16, V=1030), EUNSUPPORTED, "yuma_u16_native"),
    (dict(flags=engine.RUN_W_U16, W=P + 4), EUNSUPPORTED, "YUMA_RUN_W_U16 needs"),
])
def test_refusals_without_a_gpu_are_equal_from_run_and_graph(kw, code, text):
    run, graph = call_both(**kw)
    assert run[0] == code and text in run[1], run
    assert graph == run


def test_run_move_still_refuses_a_null_b_move():
    lib = engine.load_library()
    outs = engine.YumaOutputsC(Dn=P, C=P, I=P, B_final=P)
    opts = engine.YumaRunOptionsC(flags=0, hist_stride=1, hist_first=0)
    rc = lib.yuma_run_move(Y3, P, 2, 6, 0, 5, 8, P, P, None, None, None, ctypes.addressof(outs), None, 0, None, None,
                           P, 1 << 40, 0, ctypes.addressof(opts), None, None)
    assert rc == EINVAL and "B_move is NULL" in lib.yuma_last_error().decode()


def test_graph_handle_is_checked_after_the_options():
    lib = engine.load_library()
    outs = engine.YumaOutputsC(Dn=P, C=P, I=P, B_final=P)
    bad = engine.YumaRunOptionsC(flags=0, hist_stride=-1)
    args = (Y3, P, 0, 6, 0, 5, 8, P, P, None, None, None, ctypes.addressof(outs), None, 0, None, None, P, 3, P, P,
            1 << 40, 0)
    assert lib.yuma_graph_create_rows(None, *args, ctypes.addressof(bad)) == EINVAL
    assert "hist_stride" in lib.yuma_last_error().decode()
    ok = engine.YumaRunOptionsC()
    assert lib.yuma_graph_create_rows(None, *args, ctypes.addressof(ok)) == EINVAL
    assert "graph handle" in lib.yuma_last_error().decode()   # ... and before the sizes (N = 0)


# ---------------------------------------------------------------------------
# engine.run validates watch_rows= on the host
# ---------------------------------------------------------------------------
@pytest.fixture()
def no_device(monkeypatch):
    """Any request for the device fails the test: validation comes first."""
    def boom():
        raise AssertionError("a device was asked for before the row list was validated")
    monkeypatch.setattr(engine, "device", boom)


def run_args(variant=Y3, E=3, N=2, V=5, M=8):
    g = torch.Generator().manual_seed(1)
    W, S = torch.rand((E, N, V, M), generator=g), torch.rand((E, N, V), generator=g) + 0.5
    return variant, [engine.make_params(variant, YumaConfig())] * N, W, S


@pytest.mark.parametrize("bad,text", [
    ([], "watch_rows must"), (torch.zeros(0, dtype=torch.int32), "non-empty"), ([[0, 1]], "one-dimensional"),
    ([0, -1], "found -1"), ([5], r"\[0, V=5\): found 5"), ([0, 7, 2], "found 7"),   # (7 is a miner, no validator)
    ([0.0, 1.0], "integer validator indices"), ([True], "integer validator indices"),
    (torch.tensor([1, 5], dtype=torch.int64), "found 5"),
])
def test_run_rejects_a_bad_row_list_before_touching_the_device(no_device, bad, text):
    variant, params, W, S = run_args()
    with pytest.raises(ValueError, match=text):
        engine.run(variant, params, W, S, watch_rows=bad)
    with pytest.raises(ValueError, match=text):
        engine.RunGraph(variant, params, W, S, watch_rows=bad)


def test_run_rejects_resets_with_watch_rows_before_touching_the_device(no_device):
    variant, params, W, S = run_args()
    with pytest.raises(ValueError, match="does not combine with watch_rows"):
        engine.run(variant, params, W, S, resets=[(1, 0, 1, engine.RESET_ALWAYS)], watch_rows=[0])
    with pytest.raises(ValueError, match="does not combine with watch_rows"):
        engine.RunGraph(variant, params, W, S, resets=[(1, 0, 1, engine.RESET_ALWAYS)], watch_rows=[0])


def test_row_list_host_form():
    h = engine._watch_host([4, 0, 4], 5, "watch_rows", "validator", "V")
    assert h.dtype == torch.int64 and h.tolist() == [4, 0, 4]


# ---------------------------------------------------------------------------
# run_simulations validates bonds_validators on the host
# ---------------------------------------------------------------------------
def sim_runs():
    case = builtin_cases[0]
    return [SimulationRun(case, v, YumaConfig()) for v in ("Yuma 3.1 (Rhef+reset)", "Yuma 3 (Rhef)")]


@pytest.mark.parametrize("bad,text", [
    ([], "bonds_validators must"), ([0, -1], "found -1"), ([0.5], "integer validator indices"),
    ([0, 10**6], "index 1000000 is outside run 0"),
])
def test_run_simulations_rejects_bad_bonds_validators_before_touching_the_device(no_device, bad, text):
    with pytest.raises(ValueError, match=text):
        run_simulations(sim_runs(), bonds_validators=bad)


def test_run_simulations_checks_every_runs_validator_count(no_device):
    V = builtin_cases[0].packed_inputs()[0].shape[-2]
    with pytest.raises(ValueError, match=f"V={V} validators"):
        run_simulations(sim_runs(), bonds_validators=[0, V])


@pytest.mark.parametrize("kw,text", [
    (dict(bonds_columns=[0]), "bonds_columns"), (dict(bond_resets=[[(1, 0)], None]), "bond_resets"),
])
def test_run_simulations_rejects_the_combinations_before_touching_the_device(no_device, kw, text):
    with pytest.raises(ValueError, match=text):
        run_simulations(sim_runs(), bonds_validators=[0], **kw)


# ---------------------------------------------------------------------------
# the register report of k_bonds_rows, from the built library's code object
# ---------------------------------------------------------------------------
def test_no_rows_kernel_spills_or_uses_scratch():
    """The 16 k_bonds_rows<VARIANT, WT, SC, C> forms (Yuma 3 / Yuma 4, fp32 /
    uint16 weights, with / without a schedule, four columns / one per thread)
    report no spilled VGPR, no spilled SGPR and no scratch."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kcompare

    meta = kcompare.kernels(engine.LIB_PATH)
    rows = {k: v[2] for k, v in meta.items() if "k_bonds_rows" in k}
    assert len(rows) == 16, sorted(rows)
    assert sorted({re.search(r"k_bonds_rowsILi(\d)", k).group(1) for k in rows}) == ["3", "4"]
    fields = dict(zip(kcompare.FIELDS, range(len(kcompare.FIELDS))))
    for name, m in rows.items():
        for f in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
            assert m[fields[f]] == "0", (name, f, m)
