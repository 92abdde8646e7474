"""Bond movement per epoch, host side (no GPU): the C-ABI of yuma_run_move and
its companions, the yuma_move_native truth table, the refusals that come back
before the first launch (equal from the direct run and the graph form, in the
order the header documents), engine.settled_epoch on hand-made arrays, and the
want_move argument checks of engine.run, which raise before anything touches a
device."""

from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest
import torch

from yuma_simulation._internal import engine
from yuma_simulation._internal.yumas import YumaConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("yuma_run_move", "yuma_graph_create_move", "yuma_move_native")
RUST, Y1, Y2, Y3, Y4 = range(5)
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4
MAXV = engine.MAX_VALIDATORS


def header_code():
    text = open(os.path.join(ROOT, "include", "yuma_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def proto(name):
    return re.search(r"\b(\w+)\s+" + name + r"\s*\((.*?)\)\s*;", header_code(), flags=re.S)


def test_header_declares_the_entry_points():
    for name in NEW_FUNCTIONS:
        assert proto(name).group(1) == "int", name
    for name in NEW_FUNCTIONS[:2]:
        args = re.sub(r"\s+", " ", proto(name).group(2))
        # yuma_run_watch's arguments with B_move after B_watch
        assert "const int32_t* watch_dev, int n_watch, float* B_watch, float* B_move, void* workspace" in args
        watch = re.sub(r"\s+", " ", proto(name.replace("move", "watch")).group(2))
        assert args.replace("float* B_move, ", "") == watch
    args = [re.sub(r"\s+", " ", a).strip() for a in proto("yuma_move_native").group(2).split(",")]
    assert args == ["int variant", "int N", "int E", "int V", "int M", "const yuma_outputs_t* out", "int flags"]


def test_library_exports_and_argtypes_match_the_header():
    lib = engine.load_library()
    for name in NEW_FUNCTIONS:
        assert name in engine.EXPORTED_SYMBOLS, name
        fn = getattr(lib, name)
        n_params = len([a for a in proto(name).group(2).split(",") if a.strip()])
        assert len(fn.argtypes) == n_params, name
        assert fn.restype is ctypes.c_int
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    a, b = list(lib.yuma_run_watch.argtypes), list(lib.yuma_run_move.argtypes)
    assert b == a[:16] + [vp] + a[16:]
    a, b = list(lib.yuma_graph_create_watch.argtypes), list(lib.yuma_graph_create_move.argtypes)
    assert b == a[:17] + [vp] + a[17:]
    assert list(lib.yuma_move_native.argtypes) == [i32] * 5 + [vp, i32]
    # the records the issue leaves alone
    assert ctypes.sizeof(engine.YumaScanPlanC) == 80 and ctypes.sizeof(engine.YumaRunOptionsC) == 32


@pytest.mark.parametrize("V,M", [(5, 8), (67, 12), (MAXV, 8)])
def test_move_native_truth_table(V, M):
    N, E = 2, 6
    for variant in (Y3, Y4):
        assert engine.move_native(variant, N, E, V, M)
        assert engine.move_native(variant, N, E, V, M, want=("D", "R", "P", "T", "Sn", "bond_alpha", "alpha_ab"))
        assert not engine.move_native(variant, N, E, V, 10)             # the scalar form
        assert not engine.move_native(variant, N, E, V, M, shared_inputs=True)
        assert not engine.move_native(variant, N, E, V, M, True)        # a history in the same run
        for name in ("Wn", "Wc", "Wb", "B_inst", "Tv"):
            assert not engine.move_native(variant, N, E, V, M, want=(name,)), name
        assert not engine.move_native(variant, N, E, MAXV + 1, M)
        assert not engine.move_native(variant, 0, E, V, M) and not engine.move_native(variant, N, 0, V, M)
        # with uint16 weights it follows yuma_u16_native
        assert engine.move_native(variant, N, E, V, M, w_u16=True) == engine.u16_native(variant, N, E, V, M)
        # with a schedule: where yuma_sched_native holds as well (P / T are the schedule's own refusals)
        assert engine.sched_native(variant, N, E, 2, V, M)
        assert engine.move_native(variant, N, E, V, M, want=("P",)) and not engine.sched_native(
            variant, N, E, 2, V, M, want=("P",))
    for variant in (RUST, Y1, Y2):
        assert not engine.move_native(variant, N, E, V, M)
    assert not engine.move_native(7, N, E, V, M)


def test_move_native_cases_reach_the_flat_scans():
    """The native set is the calls plan_scan sends to the flat history-less shapes."""
    for variant in (Y3, Y4):
        for N, V, M in ((2, 5, 8), (2, 67, 12), (1, MAXV, 8), (64, 512, 8), (3, 1030, 260)):
            assert engine.move_native(variant, N, 6, V, M)
            plan = engine.scan_plan(variant, N, 6, V, M)
            assert plan.form == "k_bonds_elem" and plan.shape in ("flat1", "flat2") and plan.vector_form, plan
            assert plan.rq and not plan.hist and plan.dpl == "QTE", plan


# ---------------------------------------------------------------------------
# refusals before the first launch: no GPU, no HIP call. The pointers are never
# dereferenced (any non-null value stands for device memory).
# ---------------------------------------------------------------------------
P = 0x1000  # a non-null "device pointer"


def call_both(variant=Y3, N=2, E=6, K=0, V=5, M=8, sched=None, watch=None, n_watch=0, b_watch=None, b_move=P,
              ws_bytes=None, flags=0, hist=None, W=P, want=()):
    """(code, text) of yuma_run_move and of yuma_graph_create_move."""
    lib = engine.load_library()
    outs = engine.YumaOutputsC(Dn=P, C=P, I=P, B_final=P, B_hist=hist, **{k: P for k in want})
    opts = engine.YumaRunOptionsC(flags=flags, hist_stride=1, hist_first=0)
    if ws_bytes is None:
        ws_bytes = 1 << 40
    common = (variant, P, N, E, K, V, M, W, P, sched, None, None, ctypes.addressof(outs), watch, n_watch, b_watch,
              b_move, P, ws_bytes, 0, ctypes.addressof(opts))
    rc_run = lib.yuma_run_move(*common, None, None)
    msg_run = lib.yuma_last_error().decode()
    h = ctypes.c_void_p()
    rc_graph = lib.yuma_graph_create_move(ctypes.byref(h), *common)
    msg_graph = lib.yuma_last_error().decode()
    assert h.value is None
    return (rc_run, msg_run), (rc_graph, msg_graph)


WATCH = dict(watch=P, n_watch=3, b_watch=P)


@pytest.mark.parametrize("kw,code,text", [
    (dict(N=0), EINVAL, "sizes must be positive"),
    (dict(V=MAXV + 1), EUNSUPPORTED, "YUMA_MAX_VALIDATORS"),
    (dict(W=None), EINVAL, "null params"),
    (dict(sched=P, K=0), EINVAL, "K=0"),          # exactly one of sched_dev / K
    (dict(sched=None, K=3), EINVAL, "K=3"),
    # a watch list: n_watch != 0 or either pointer given; then yuma_run_watch's own checks
    (dict(watch=P, n_watch=0, b_watch=P), EINVAL, "n_watch=0"),
    (dict(watch=P, n_watch=0), EINVAL, "n_watch=0"),
    (dict(n_watch=-2), EINVAL, "n_watch=-2"),
    (dict(n_watch=3), EINVAL, "watch list or B_watch is NULL"),
    (dict(watch=P, n_watch=3), EINVAL, "watch list or B_watch is NULL"),
    # B_move beside the watch-pointer checks: after them, before the workspace size
    (dict(b_move=None), EINVAL, "B_move is NULL"),
    (dict(b_move=None, n_watch=3), EINVAL, "watch list or B_watch is NULL"),
    (dict(b_move=None, ws_bytes=16), EINVAL, "B_move is NULL"),
    (dict(b_move=None, variant=Y1), EINVAL, "B_move is NULL"),
    (dict(sched=P, K=0, b_move=None), EINVAL, "K=0"),
    # "no watch list" (n_watch = 0, NULL list, NULL B_watch) is accepted up to the workspace check
    (dict(ws_bytes=16), EWORKSPACE, "workspace"),
    (dict(ws_bytes=16, **WATCH), EWORKSPACE, "workspace"),
    (dict(ws_bytes=16, variant=Y1), EWORKSPACE, "workspace"),   # ... which comes before "not native"
    # the schedule's refusal, then the watch list's, then the movement's
    (dict(sched=P, K=3, M=10), EUNSUPPORTED, "yuma_sched_native"),
    (dict(variant=Y1, **WATCH), EUNSUPPORTED, "yuma_watch_native"),
    (dict(variant=Y4, flags=engine.RUN_SHARED_INPUTS, **WATCH), EUNSUPPORTED, "yuma_watch_native"),
    (dict(variant=RUST), EUNSUPPORTED, "yuma_move_native"),
    (dict(variant=Y1), EUNSUPPORTED, "yuma_move_native"),
    (dict(variant=Y2), EUNSUPPORTED, "yuma_move_native"),
    (dict(M=10), EUNSUPPORTED, "yuma_move_native"),
    (dict(M=10, **WATCH), EUNSUPPORTED, "yuma_move_native"),     # the watch kernel takes any M; the movement does not
    (dict(flags=engine.RUN_SHARED_INPUTS), EUNSUPPORTED, "yuma_move_native"),
    (dict(hist=P), EUNSUPPORTED, "yuma_move_native"),
    (dict(hist=P, **WATCH), EUNSUPPORTED, "yuma_move_native"),
    (dict(want=("Wn",)), EUNSUPPORTED, "yuma_move_native"),
    (dict(want=("Tv",)), EUNSUPPORTED, "yuma_move_native"),
    (dict(W=P + 4), EUNSUPPORTED, "needs the vector form"),       # native by its sizes, W off its alignment
    # ... and before YUMA_RUN_HIST_BF16 / YUMA_RUN_W_U16
    (dict(flags=engine.RUN_HIST_BF16), EUNSUPPORTED, "yuma_move_native"),
    (dict(flags=engine.RUN_W_U16, V=MAXV), EUNSUPPORTED, "yuma_move_native"),
])
def test_refusals_without_a_gpu_are_equal_from_run_and_graph(kw, code, text):
    run, graph = call_both(**kw)
    assert run[0] == code and text in run[1], run
    assert graph == run


def test_run_watch_still_refuses_an_empty_list():
    lib = engine.load_library()
    outs = engine.YumaOutputsC(Dn=P, C=P, I=P, B_final=P)
    opts = engine.YumaRunOptionsC(flags=0, hist_stride=1, hist_first=0)
    rc = lib.yuma_run_watch(Y3, P, 2, 6, 0, 5, 8, P, P, None, None, None, ctypes.addressof(outs), None, 0, None, P,
                            1 << 40, 0, ctypes.addressof(opts), None, None)
    assert rc == EINVAL and "n_watch=0" in lib.yuma_last_error().decode()


def test_graph_handle_is_checked_after_the_options():
    lib = engine.load_library()
    outs = engine.YumaOutputsC(Dn=P, C=P, I=P, B_final=P)
    bad = engine.YumaRunOptionsC(flags=0, hist_stride=-1)
    args = (Y3, P, 2, 6, 0, 5, 8, P, P, None, None, None, ctypes.addressof(outs), None, 0, None, P, P, 1 << 40, 0)
    assert lib.yuma_graph_create_move(None, *args, ctypes.addressof(bad)) == EINVAL
    assert "hist_stride" in lib.yuma_last_error().decode()
    ok = engine.YumaRunOptionsC()
    assert lib.yuma_graph_create_move(None, *args, ctypes.addressof(ok)) == EINVAL
    assert "graph handle" in lib.yuma_last_error().decode()


def test_scan_plan_reports_the_plan_without_the_movement():
    """yuma_scan_plan_t is untouched: the fields the binding has always read."""
    names = [n for n, _ in engine.YumaScanPlanC._fields_]
    assert "mv" not in names and len(names) == 19


# ---------------------------------------------------------------------------
# engine.settled_epoch: pure torch / numpy, on CPU tensors
# ---------------------------------------------------------------------------
def mv(moved, size=None):
    moved = torch.tensor(moved, dtype=torch.float32)
    size = torch.ones_like(moved) if size is None else torch.tensor(size, dtype=torch.float32)
    return torch.stack([moved, size], dim=-1)


def test_settled_epoch_on_hand_made_arrays():
    nan = float("nan")
    # settles at 0; never settles (E); dips below tol and rises again
    assert engine.settled_epoch(mv([0.0, 0.0, 0.0]), 1e-6).item() == 0
    assert engine.settled_epoch(mv([1.0, 1.0, 1.0]), 1e-6).item() == 3
    assert engine.settled_epoch(mv([1.0, 0.0, 0.5, 0.0, 0.0]), 0.1).item() == 3
    assert engine.settled_epoch(mv([1.0, 0.5, 0.1, 0.05]), 0.1).item() == 2    # <= tol counts
    # a NaN never counts as settled: in the tail nothing settles, before the tail it only delays
    assert engine.settled_epoch(mv([1.0, 0.0, 0.0, nan]), 0.1).item() == 4
    assert engine.settled_epoch(mv([1.0, nan, 0.0, 0.0]), 0.1).item() == 2
    assert engine.settled_epoch(mv([0.0, 0.0], [nan, nan]), 0.1, relative=True).tolist() == 2
    # relative against absolute: Yuma 3's 2^64 scale
    big = 2.0 ** 64
    m = mv([big, big * 1e-3, big * 1e-7, big * 1e-8], [big] * 4)
    assert engine.settled_epoch(m, 1e-6).item() == 4
    assert engine.settled_epoch(m, 1e-6, relative=True).item() == 2
    assert engine.settled_epoch(mv([0.0, 0.0], [0.0, 0.0]), 1e-6, relative=True).item() == 0  # 0 <= tol * 0
    # N > 1 with different answers; the result is one int64 per scenario
    m = mv([[1.0, 0.0, 1.0], [0.5, 0.0, 1.0], [0.0, 0.0, nan], [0.0, 0.0, 0.0]])
    r = engine.settled_epoch(m, 0.1)
    assert r.dtype == torch.int64 and r.tolist() == [2, 0, 3]
    # numpy in, and no epochs at all
    assert engine.settled_epoch(m.numpy(), 0.1).tolist() == [2, 0, 3]
    assert engine.settled_epoch(torch.zeros((0, 2, 2)), 0.1).tolist() == [0, 0]
    with pytest.raises(ValueError, match="B_move"):
        engine.settled_epoch(torch.zeros((3, 2, 3)), 0.1)


def test_move_from_history_is_the_definition():
    g = torch.Generator().manual_seed(3)
    hist = torch.rand((5, 2, 3, 4), generator=g) - 0.5
    b0 = torch.rand((2, 3, 4), generator=g)
    for init in (None, b0):
        full = torch.cat([torch.zeros_like(hist[:1]) if init is None else init[None], hist])
        got = engine.move_from_history(hist, init)
        assert got.shape == (5, 2, 2) and got.dtype == torch.float32
        assert torch.equal(got[..., 0], (full[1:] - full[:-1]).abs().amax((-2, -1)))
        assert torch.equal(got[..., 1], hist.abs().amax((-2, -1)))


# ---------------------------------------------------------------------------
# engine.run validates want_move on the host
# ---------------------------------------------------------------------------
@pytest.fixture()
def no_device(monkeypatch):
    """Any request for the device fails the test: validation comes first."""
    def boom():
        raise AssertionError("a device was asked for before want_move was validated")
    monkeypatch.setattr(engine, "device", boom)


def run_args(E=3, N=2, V=5, M=8):
    g = torch.Generator().manual_seed(1)
    W, S = torch.rand((E, N, V, M), generator=g), torch.rand((E, N, V), generator=g) + 0.5
    return Y3, [engine.make_params(Y3, YumaConfig())] * N, W, S


def test_run_rejects_bad_want_move_arguments_before_touching_the_device(no_device):
    variant, params, W, S = run_args()
    for bad in (1, "yes", None, [True]):
        with pytest.raises(ValueError, match="want_move"):
            engine.run(variant, params, W, S, want_move=bad)
    with pytest.raises(ValueError, match="want_move"):
        engine.run(variant, params, W[:1], S[:1], want_move=True, single_call=True)
    with pytest.raises(ValueError, match="want_move"):
        engine.RunGraph(variant, params, W, S, want_move=1)


def test_run_result_has_the_new_field_with_a_default():
    r = engine.RunResult(None, None, None, None, None, {})
    assert r.B_move is None
