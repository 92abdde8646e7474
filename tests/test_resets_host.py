"""Bond reset events, host side (no GPU): the C-ABI of yuma_run_resets and its
companions, the yuma_resets_native truth table beside the older predicates, the
refusals that come back before the first launch (equal from the direct run and
the graph form, in the order the header documents), and the argument checks of
engine.run(resets=) and run_simulations(bond_resets=), which raise before
anything touches a device."""

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
NEW_FUNCTIONS = ("yuma_run_resets", "yuma_graph_create_resets", "yuma_resets_native", "yuma_workspace_bytes_resets")
RUST, Y1, Y2, Y3, Y4 = range(5)
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4
MAXV = engine.MAX_VALIDATORS
ALWAYS, IF_ZERO = engine.RESET_ALWAYS, engine.RESET_IF_ZERO_CONSENSUS


def header_code():
    text = open(os.path.join(ROOT, "include", "yuma_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def proto(name):
    return re.search(r"\b(\w+)\s+" + name + r"\s*\((.*?)\)\s*;", header_code(), flags=re.S)


def test_header_declares_the_entry_points_and_the_event_record():
    for name in NEW_FUNCTIONS[:3]:
        assert proto(name).group(1) == "int", name
    assert proto("yuma_workspace_bytes_resets").group(1) == "size_t"
    for name in NEW_FUNCTIONS[:2]:
        args = re.sub(r"\s+", " ", proto(name).group(2))
        # yuma_run_opts's arguments with the list and its length after `out`
        assert "const yuma_outputs_t* out, const yuma_reset_event_t* events_dev, int n_events, void* workspace" in args
        opts = re.sub(r"\s+", " ", proto(name.replace("resets", "opts")).group(2))
        assert args.replace("const yuma_reset_event_t* events_dev, int n_events, ", "") == opts
    args = [re.sub(r"\s+", " ", a).strip() for a in proto("yuma_resets_native").group(2).split(",")]
    assert args == ["int variant", "int N", "int E", "int V", "int M", "const yuma_outputs_t* out", "int flags"]
    body = re.search(r"typedef struct yuma_reset_event \{([^}]*)\}\s*yuma_reset_event_t;", header_code()).group(1)
    assert re.findall(r"\bint32_t\s+(\w+)\s*;", body) == [n for n, _ in engine.YumaResetEventC._fields_]
    assert [n for n, _ in engine.YumaResetEventC._fields_] == ["epoch", "scenario", "column", "mode"]
    assert ctypes.sizeof(engine.YumaResetEventC) == 16


def test_library_exports_and_argtypes_match_the_header():
    lib = engine.load_library()
    for name in NEW_FUNCTIONS:
        assert name in engine.EXPORTED_SYMBOLS, name
        fn = getattr(lib, name)
        n_params = len([a for a in proto(name).group(2).split(",") if a.strip()])
        assert len(fn.argtypes) == n_params, name
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    a, b = list(lib.yuma_run_opts.argtypes), list(lib.yuma_run_resets.argtypes)
    assert b == a[:11] + [vp, i32] + a[11:]
    a, b = list(lib.yuma_graph_create_opts.argtypes), list(lib.yuma_graph_create_resets.argtypes)
    assert b == a[:12] + [vp, i32] + a[12:]
    assert list(lib.yuma_resets_native.argtypes) == [i32] * 5 + [vp, i32]
    assert lib.yuma_resets_native.restype is ctypes.c_int
    assert lib.yuma_workspace_bytes_resets.restype is ctypes.c_size_t
    assert list(lib.yuma_workspace_bytes_resets.argtypes) == list(lib.yuma_workspace_bytes.argtypes)
    # the records the issue leaves alone
    assert ctypes.sizeof(engine.YumaScanPlanC) == 80 and ctypes.sizeof(engine.YumaRunOptionsC) == 32
    assert "rl" not in [n for n, _ in engine.YumaScanPlanC._fields_]


@pytest.mark.parametrize("V,M", [(5, 8), (67, 12), (33, 68), (5, 1032), (MAXV, 8)])
def test_resets_native_truth_table(V, M):
    N, E = 2, 6
    for variant in (Y3, Y4):
        # both sides of each condition
        assert engine.resets_native(variant, N, E, V, M)
        assert engine.resets_native(variant, N, E, V, M, True)                # an fp32 history, dense or strided
        assert engine.resets_native(variant, N, E, V, M, want=("D", "R", "P", "T", "Sn", "bond_alpha", "alpha_ab"))
        assert not engine.resets_native(variant, N, E, V, M + 2)              # the scalar form
        assert not engine.resets_native(variant, N, E, V, M, shared_inputs=True)
        assert not engine.resets_native(variant, N, E, V, M, w_u16=True)
        assert not engine.resets_native(variant, N, E, V, M, True, hist_bf16=True)
        for name in ("Wn", "Wc", "Wb", "B_inst", "Tv"):
            assert not engine.resets_native(variant, N, E, V, M, want=(name,)), name
        assert not engine.resets_native(variant, N, E, MAXV + 1, M)
        assert not engine.resets_native(variant, 0, E, V, M) and not engine.resets_native(variant, N, 0, V, M)
        assert not engine.resets_native(variant, N, E, 0, M) and not engine.resets_native(variant, N, E, V, 0)
    for variant in (RUST, Y1, Y2, 7, -1):
        assert not engine.resets_native(variant, N, E, V, M)


@pytest.mark.parametrize("N,V,M,hist,shape", [
    (2, 5, 260, False, "flat1"), (64, 512, 8, False, "flat2"), (2, 33, 68, True, "tile_hist"),
    (1, 5, 1032, True, "wide"), (1, 1030, 8, False, "flat1"), (1, 1030, 8, True, "tile_hist"),
    (1, MAXV, 8, False, "flat2"),
])
def test_native_cases_reach_the_four_shapes(N, V, M, hist, shape):
    """The native set is the calls plan_scan sends to the wide, tile-history and flat shapes."""
    for variant in (Y3, Y4):
        assert engine.resets_native(variant, N, 6, V, M, hist)
        for kw in ({}, dict(hist_stride=2, hist_first=1)):
            plan = engine.scan_plan(variant, N, 6, V, M, hist, **kw)
            assert plan.form == "k_bonds_elem" and plan.shape == shape and plan.vector_form, plan
            assert plan.rq == (not hist) and not plan.hist_bf16 and not plan.sc and not plan.w_u16, plan


def test_older_predicates_keep_their_answers():
    """The same arguments through the pre-existing predicates, beside the new one: the table their own tests hold."""
    N, E = 2, 6
    for variant in (Y3, Y4):
        for V, M in ((5, 8), (67, 12), (MAXV, 8)):
            assert engine.resets_native(variant, N, E, V, M) and engine.resets_native(variant, N, E, V, M, True)
            assert engine.move_native(variant, N, E, V, M) and not engine.move_native(variant, N, E, V, M, True)
            assert engine.sched_native(variant, N, E, 2, V, M) and not engine.sched_native(variant, N, E, 2, V, M + 2)
            assert engine.watch_native(variant, N, E, V, M + 1, 3)
            assert engine.hist_bf16_native(variant, N, E, V, M) and not engine.hist_bf16_native(variant, N, E, V, M + 2)
            assert engine.u16_native(variant, N, E, V, M) == (V <= engine.REG_VALIDATORS)
    for variant in (RUST, Y1, Y2):
        assert not engine.resets_native(variant, N, E, 5, 8)
        assert not engine.move_native(variant, N, E, 5, 8) and not engine.sched_native(variant, N, E, 2, 5, 8)
        assert not engine.watch_native(variant, N, E, 5, 8, 3) and not engine.u16_native(variant, N, E, 5, 8)


@pytest.mark.parametrize("variant,N,E,V,M", [(Y3, 2, 6, 5, 8), (Y4, 1, 5, 5, 1032), (Y3, 256, 100, 64, 4096), (Y1, 2, 3, 70, 10)])
def test_workspace_bytes_resets(variant, N, E, V, M):
    lib = engine.load_library()
    for full in (0, 1):
        plain = lib.yuma_workspace_bytes(variant, N, E, V, M, full)
        table = lib.yuma_workspace_bytes_resets(variant, N, E, V, M, full) - plain
        assert table >= E * N * ((M + 7) // 8)       # one bit per (epoch, scenario, column)
        assert table < E * N * ((M + 7) // 8) + 1024  # ... and padding only
    assert lib.yuma_workspace_bytes_resets(variant, 0, E, V, M, 0) == 0


# ---------------------------------------------------------------------------
# refusals before the first launch: no GPU, no HIP call. The pointers are never
# dereferenced (any non-null value stands for device memory).
# ---------------------------------------------------------------------------
P = 0x1000  # a non-null "device pointer"


def call_both(variant=Y3, N=2, E=6, V=5, M=8, events=P, n_events=3, ws_bytes=None, flags=0, hist=None, W=P, want=(),
              stride=1, out=True):
    """(code, text) of yuma_run_resets and of yuma_graph_create_resets."""
    lib = engine.load_library()
    outs = engine.YumaOutputsC(Dn=P, C=P, I=P, B_final=P, B_hist=hist, **{k: P for k in want})
    opts = engine.YumaRunOptionsC(flags=flags, hist_stride=stride, hist_first=0)
    if ws_bytes is None:
        ws_bytes = 1 << 40
    common = (variant, P, N, E, V, M, W, P, None, None, ctypes.addressof(outs) if out else None, events, n_events,
              P, ws_bytes, 0, ctypes.addressof(opts))
    rc_run = lib.yuma_run_resets(*common, None, None)
    msg_run = lib.yuma_last_error().decode()
    h = ctypes.c_void_p()
    rc_graph = lib.yuma_graph_create_resets(ctypes.byref(h), *common)
    msg_graph = lib.yuma_last_error().decode()
    assert h.value is None
    return (rc_run, msg_run), (rc_graph, msg_graph)


def ws_plain(variant=Y3, N=2, E=6, V=5, M=8):
    return engine.load_library().yuma_workspace_bytes(variant, N, E, V, M, 0)


@pytest.mark.parametrize("kw,code,text", [
    # 1. the options
    (dict(flags=64), EINVAL, "unknown run flags"),
    (dict(stride=-1, N=0), EINVAL, "hist_stride"),
    # 3. sizes
    (dict(N=0, W=None), EINVAL, "sizes must be positive"),
    (dict(V=MAXV + 1, W=None), EUNSUPPORTED, "YUMA_MAX_VALIDATORS"),
    # 4. NULL pointers, before the event list's own checks
    (dict(W=None, n_events=-1), EINVAL, "null params"),
    (dict(out=False, events=None), EINVAL, "null params"),
    # 5. n_events < 0, then n_events > 0 with a NULL list; both before the workspace size
    (dict(n_events=-1), EINVAL, "n_events=-1"),
    (dict(n_events=-1, events=None, ws_bytes=16), EINVAL, "n_events=-1"),
    (dict(events=None, n_events=3), EINVAL, "NULL event list"),
    (dict(events=None, n_events=3, ws_bytes=16, variant=Y1), EINVAL, "NULL event list"),
    # 6. the workspace size: yuma_workspace_bytes is too small once there is a list, and comes before "not native"
    (dict(ws_bytes=16), EWORKSPACE, "workspace"),
    (dict(ws_bytes=ws_plain()), EWORKSPACE, "workspace"),
    (dict(ws_bytes=16, variant=Y1), EWORKSPACE, "workspace"),
    (dict(ws_bytes=16, M=10), EWORKSPACE, "workspace"),
    # 7. not native, then not in vector form
    (dict(variant=RUST), EUNSUPPORTED, "yuma_resets_native"),
    (dict(variant=Y1), EUNSUPPORTED, "yuma_resets_native"),
    (dict(variant=Y2), EUNSUPPORTED, "yuma_resets_native"),
    (dict(M=10), EUNSUPPORTED, "yuma_resets_native"),
    (dict(M=10, W=P + 4), EUNSUPPORTED, "yuma_resets_native"),
    (dict(flags=engine.RUN_SHARED_INPUTS), EUNSUPPORTED, "yuma_resets_native"),
    (dict(flags=engine.RUN_W_U16), EUNSUPPORTED, "yuma_resets_native"),
    (dict(flags=engine.RUN_HIST_BF16, hist=P), EUNSUPPORTED, "yuma_resets_native"),
    (dict(flags=engine.RUN_HIST_BF16), EUNSUPPORTED, "yuma_resets_native"),   # before "without out->B_hist"
    (dict(want=("Wn",)), EUNSUPPORTED, "yuma_resets_native"),
    (dict(want=("Tv",)), EUNSUPPORTED, "yuma_resets_native"),
    (dict(W=P + 4), EUNSUPPORTED, "need the vector form"),
    (dict(hist=P + 4), EUNSUPPORTED, "need the vector form"),
    # an empty list that is present (n_events = 0, a pointer) is a run with events: the table's workspace
    (dict(n_events=0, ws_bytes=ws_plain()), EWORKSPACE, "workspace"),
    (dict(n_events=0, variant=Y1), EUNSUPPORTED, "yuma_resets_native"),
])
def test_refusals_without_a_gpu_are_equal_from_run_and_graph(kw, code, text):
    run, graph = call_both(**kw)
    assert run[0] == code and text in run[1], run
    assert graph == run


def test_no_events_is_yuma_run_opts():
    """n_events = 0 with a NULL list: yuma_run_opts's own checks and workspace size, nothing about events."""
    lib = engine.load_library()
    outs = engine.YumaOutputsC(Dn=P, C=P, I=P, B_final=P)
    opts = engine.YumaRunOptionsC()
    for variant, M, ws in ((Y3, 8, 16), (Y1, 10, 16), (Y3, 8, ws_plain() - 1)):
        rc = lib.yuma_run_resets(variant, P, 2, 6, 5, M, P, P, None, None, ctypes.addressof(outs), None, 0, P, ws, 0,
                                 ctypes.addressof(opts), None, None)
        msg = lib.yuma_last_error().decode()
        rc2 = lib.yuma_run_opts(variant, P, 2, 6, 5, M, P, P, None, None, ctypes.addressof(outs), P, ws, 0,
                                ctypes.addressof(opts), None, None)
        assert (rc, msg) == (rc2, lib.yuma_last_error().decode()) and rc == EWORKSPACE


def test_graph_handle_is_checked_after_the_options():
    lib = engine.load_library()
    outs = engine.YumaOutputsC(Dn=P, C=P, I=P, B_final=P)
    bad = engine.YumaRunOptionsC(flags=0, hist_stride=-1)
    args = (Y3, P, 0, 6, 5, 8, P, P, None, None, ctypes.addressof(outs), P, 3, P, 1 << 40, 0)
    assert lib.yuma_graph_create_resets(None, *args, ctypes.addressof(bad)) == EINVAL
    assert "hist_stride" in lib.yuma_last_error().decode()
    ok = engine.YumaRunOptionsC()
    assert lib.yuma_graph_create_resets(None, *args, ctypes.addressof(ok)) == EINVAL
    assert "graph handle" in lib.yuma_last_error().decode()   # ... and before the sizes (N = 0)


# ---------------------------------------------------------------------------
# engine.run validates resets= on the host
# ---------------------------------------------------------------------------
@pytest.fixture()
def no_device(monkeypatch):
    """Any request for the device fails the test: validation comes first."""
    def boom():
        raise AssertionError("a device was asked for before resets= was validated")
    monkeypatch.setattr(engine, "device", boom)


def run_args(variant=Y3, E=3, N=2, V=5, M=8):
    g = torch.Generator().manual_seed(1)
    W, S = torch.rand((E, N, V, M), generator=g), torch.rand((E, N, V), generator=g) + 0.5
    return variant, [engine.make_params(variant, YumaConfig())] * N, W, S


@pytest.mark.parametrize("bad,text", [
    ([(3, 0, 1, ALWAYS)], "epoch 3"), ([(-1, 0, 1, ALWAYS)], "epoch -1"),
    ([(1, 2, 1, ALWAYS)], "scenario 2"), ([(1, -1, 1, ALWAYS)], "scenario -1"),
    ([(1, 0, 8, ALWAYS)], "column 8"), ([(1, 0, -2, IF_ZERO)], "column -2"),
    ([(1, 0, 1, 0)], "mode 0"), ([(1, 0, 1, 3)], "mode 3"),
    ([(0, 0, 0, ALWAYS), (1, 1, 7, IF_ZERO), (1, 1, 9, IF_ZERO)], r"resets\[2\]"),
    ([(1, 0, 1)], "shape"), ([1, 0, 1, 1], "shape"), ([(1.0, 0.0, 1.0, 1.0)], "integers"),
    (torch.tensor([[1, 0, 8, 1]], dtype=torch.int32), "column 8"),     # a CPU tensor is a host list
])
def test_run_rejects_bad_events_before_touching_the_device(no_device, bad, text):
    variant, params, W, S = run_args()
    with pytest.raises(ValueError, match=text):
        engine.run(variant, params, W, S, resets=bad)
    with pytest.raises(ValueError, match=text):
        engine.RunGraph(variant, params, W, S, resets=bad)


def test_host_events_accept_the_whole_range():
    ev = [(0, 0, -1, ALWAYS), (2, 1, 7, IF_ZERO), (2, 1, 7, IF_ZERO), (1, 0, 0, ALWAYS)]
    h = engine._resets_host(ev, 2, 3, 8)
    assert h.dtype == torch.int64 and h.tolist() == [list(e) for e in ev]
    assert engine._resets_host([], 2, 3, 8).shape == (0, 4)
    assert engine._resets_host(torch.tensor(ev, dtype=torch.int32), 2, 3, 8).tolist() == [list(e) for e in ev]


@pytest.mark.parametrize("kw,text", [
    (dict(sched=[0, 1, 2]), "sched"), (dict(watch=[1]), "watch"), (dict(want_move=True), "want_move"),
    (dict(single_call=True), "single_call"), (dict(hist_dtype=torch.bfloat16, want_hist=True), "bfloat16"),
])
def test_run_rejects_the_combinations_before_touching_the_device(no_device, kw, text):
    variant, params, W, S = run_args()
    with pytest.raises(ValueError, match=text):
        engine.run(variant, params, W, S, resets=[(1, 0, 1, ALWAYS)], **kw)


@pytest.mark.parametrize("variant", [RUST, Y1, Y2])
def test_run_rejects_the_other_variants_before_touching_the_device(no_device, variant):
    variant, params, W, S = run_args(variant)
    with pytest.raises(ValueError, match="Yuma 3 / Yuma 4"):
        engine.run(variant, params, W, S, resets=[(1, 0, 1, ALWAYS)])
    with pytest.raises(ValueError, match="Yuma 3 / Yuma 4"):
        engine.run(variant, params, W, S, resets=[])


# ---------------------------------------------------------------------------
# run_simulations validates bond_resets on the host
# ---------------------------------------------------------------------------
def sim_runs():
    case = builtin_cases[0]
    return [SimulationRun(case, v, YumaConfig()) for v in ("Yuma 3.1 (Rhef+reset)", "Yuma 3 (Rhef)")]


@pytest.mark.parametrize("bad,text", [
    ([None], "one entry"), ("ab", "one entry"), (3, "one entry"),
    ([[(1, 0, 0)], None], "pair"), ([[(1.0, 0)], None], "pair"), ([[(True, 0)], None], "pair"), ([[5], None], "pair"),
    ([[(-1, 0)], None], "negative"), ([None, [(1, -1)]], "index -1"), ([None, [(1, 10**6)]], "index 1000000"),
])
def test_run_simulations_rejects_bad_bond_resets_before_touching_the_device(no_device, bad, text):
    runs = sim_runs()
    with pytest.raises(ValueError, match=text):
        run_simulations(runs, bond_resets=bad)


@pytest.mark.parametrize("kw,text", [
    (dict(dedup_inputs=True), "dedup_inputs"), (dict(bonds_columns=[0]), "bonds_columns"),
    (dict(bonds_movement=True), "bonds_movement"), (dict(bonds_dtype=torch.bfloat16), "bfloat16"),
])
def test_run_simulations_rejects_the_combinations_before_touching_the_device(no_device, kw, text):
    runs = sim_runs()
    with pytest.raises(ValueError, match=text):
        run_simulations(runs, bond_resets=[[(1, 0)], None], **kw)


# ---------------------------------------------------------------------------
# the register report of the RL kernels, from the built library's code object
# ---------------------------------------------------------------------------
def test_no_rl_kernel_spills_or_uses_scratch():
    """The 12 RL forms of k_bonds_elem report no spilled VGPR, no spilled SGPR
    and no scratch. Two empty asm statements steer their register classes
    (the AND mask and the table pointer's step in vector registers): a compiler
    that stops honouring them shows here, not only in profiles/resets/."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kcompare

    meta = kcompare.kernels(engine.LIB_PATH)
    forms = kcompare.elem_forms(meta, "RL")
    rl = {k: meta[k][2] for k in forms}
    assert len(rl) == 12, sorted(rl)
    assert sorted({variant for variant, _, _ in forms.values()}) == ["3", "4"]
    fields = dict(zip(kcompare.FIELDS, range(len(kcompare.FIELDS))))
    for name, m in rl.items():
        for f in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
            assert m[fields[f]] == "0", (name, f, m)
        assert m[fields["kernarg_segment_size"]] == "224", (name, m)   # BondArgs' 216 bytes and the table pointer
