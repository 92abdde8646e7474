"""Watched bond columns, host side (no GPU): the C-ABI of yuma_run_watch and
its companions, the yuma_watch_native truth table, the refusals that come back
before the first launch (equal from the direct run and the graph form), and the
watch-list validation of engine.run / run_simulations, which raises before
anything touches a device."""

from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest
import torch

from yuma_simulation._internal import engine
from yuma_simulation._internal.cases import cases as builtin_cases
from yuma_simulation._internal.simulation_utils import SimulationRun, run_simulations
from yuma_simulation._internal.yumas import YumaConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("yuma_run_watch", "yuma_graph_create_watch", "yuma_watch_native")
RUST, Y1, Y2, Y3, Y4 = range(5)
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4


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
        # the three new arguments follow `out`, in yuma_run_sched's argument order
        assert "const yuma_outputs_t* out, const int32_t* watch_dev, int n_watch, float* B_watch, void* workspace" in args
        assert "const int32_t* sched_dev" in args and "int K" in args and "const yuma_run_options_t* opts" in args


def test_library_exports_and_argtypes_match_the_header():
    lib = engine.load_library()
    for name in NEW_FUNCTIONS:
        assert name in engine.EXPORTED_SYMBOLS, name
        fn = getattr(lib, name)
        n_params = len([a for a in proto(name).group(2).split(",") if a.strip()])
        assert len(fn.argtypes) == n_params, name
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    a, b = list(lib.yuma_run_sched.argtypes), list(lib.yuma_run_watch.argtypes)
    assert b == a[:13] + [vp, i32, vp] + a[13:]
    a, b = list(lib.yuma_graph_create_sched.argtypes), list(lib.yuma_graph_create_watch.argtypes)
    assert b == a[:14] + [vp, i32, vp] + a[14:]
    assert list(lib.yuma_watch_native.argtypes) == [i32] * 7


@pytest.mark.parametrize("V,M", [(5, 8), (9, 10), (67, 12), (engine.MAX_VALIDATORS, 7)])
def test_watch_native_truth_table(V, M):
    N, E = 2, 6
    for variant in (Y3, Y4):
        for nw in (1, 3, 64):
            assert engine.watch_native(variant, N, E, V, M, nw)
        assert not engine.watch_native(variant, N, E, V, M, 3, shared_inputs=True)
        assert not engine.watch_native(variant, N, E, V, M, 0)
        # with uint16 weights it follows yuma_u16_native
        assert engine.watch_native(variant, N, E, V, M, 3, w_u16=True) == engine.u16_native(variant, N, E, V, M)
    for variant in (RUST, Y1, Y2):
        assert not engine.watch_native(variant, N, E, V, M, 3)
        assert not engine.watch_native(variant, N, E, V, M, 3, shared_inputs=True)
    assert not engine.watch_native(Y3, N, E, engine.MAX_VALIDATORS + 1, M, 3)


# ---------------------------------------------------------------------------
# refusals before the first launch: no GPU, no HIP call. The pointers are never
# dereferenced (any non-null value stands for device memory).
# ---------------------------------------------------------------------------
P = 0x1000  # a non-null "device pointer"


def call_both(variant=Y3, N=2, E=6, K=0, V=5, M=8, sched=None, watch=P, n_watch=3, b_watch=P, ws_bytes=None,
              flags=0):
    """(code, text) of yuma_run_watch and of yuma_graph_create_watch."""
    lib = engine.load_library()
    outs = engine.YumaOutputsC(Dn=P, C=P, I=P, B_final=P)
    opts = engine.YumaRunOptionsC(flags=flags, hist_stride=1, hist_first=0)
    if ws_bytes is None:
        ws_bytes = 1 << 40
    common = (variant, P, N, E, K, V, M, P, P, sched, None, None, ctypes.addressof(outs), watch, n_watch, b_watch,
              P, ws_bytes, 0, ctypes.addressof(opts))
    rc_run = lib.yuma_run_watch(*common, None, None)
    msg_run = lib.yuma_last_error().decode()
    h = ctypes.c_void_p()
    rc_graph = lib.yuma_graph_create_watch(ctypes.byref(h), *common)
    msg_graph = lib.yuma_last_error().decode()
    assert h.value is None
    return (rc_run, msg_run), (rc_graph, msg_graph)


@pytest.mark.parametrize("kw,code,text", [
    (dict(n_watch=0), EINVAL, "n_watch=0"),
    (dict(n_watch=-2), EINVAL, "n_watch=-2"),
    (dict(watch=None), EINVAL, "watch list or B_watch is NULL"),
    (dict(b_watch=None), EINVAL, "watch list or B_watch is NULL"),
    (dict(sched=P, K=0), EINVAL, "K=0"),          # exactly one of sched_dev / K
    (dict(sched=None, K=3), EINVAL, "K=3"),
    (dict(n_watch=0, watch=None), EINVAL, "n_watch=0"),   # the count is tested before the pointers
    (dict(variant=RUST), EUNSUPPORTED, "yuma_watch_native"),
    (dict(variant=Y1), EUNSUPPORTED, "yuma_watch_native"),
    (dict(variant=Y2), EUNSUPPORTED, "yuma_watch_native"),
    (dict(variant=Y4, flags=engine.RUN_SHARED_INPUTS), EUNSUPPORTED, "yuma_watch_native"),
    (dict(sched=P, K=3, M=10), EUNSUPPORTED, "yuma_sched_native"),  # the schedule's own refusal comes first
    (dict(ws_bytes=16), EWORKSPACE, "workspace"),
    (dict(n_watch=0, ws_bytes=16), EINVAL, "n_watch=0"),  # ... and the list before the workspace size
])
def test_refusals_without_a_gpu_are_equal_from_run_and_graph(kw, code, text):
    run, graph = call_both(**kw)
    assert run[0] == code and text in run[1], run
    assert graph == run


def test_graph_handle_is_checked_after_the_options():
    lib = engine.load_library()
    outs = engine.YumaOutputsC(Dn=P, C=P, I=P, B_final=P)
    bad = engine.YumaRunOptionsC(flags=0, hist_stride=-1)
    args = (Y3, P, 2, 6, 0, 5, 8, P, P, None, None, None, ctypes.addressof(outs), P, 3, P, P, 1 << 40, 0)
    assert lib.yuma_graph_create_watch(None, *args, ctypes.addressof(bad)) == EINVAL
    assert "hist_stride" in lib.yuma_last_error().decode()
    ok = engine.YumaRunOptionsC()
    assert lib.yuma_graph_create_watch(None, *args, ctypes.addressof(ok)) == EINVAL
    assert "graph handle" in lib.yuma_last_error().decode()


# ---------------------------------------------------------------------------
# engine.run / run_simulations validate the list on the host
# ---------------------------------------------------------------------------
@pytest.fixture()
def no_device(monkeypatch):
    """Any request for the device fails the test: validation comes first."""
    def boom():
        raise AssertionError("a device was asked for before the watch list was validated")
    monkeypatch.setattr(engine, "device", boom)


def run_args(E=3, N=2, V=5, M=8):
    g = torch.Generator().manual_seed(1)
    W, S = torch.rand((E, N, V, M), generator=g), torch.rand((E, N, V), generator=g) + 0.5
    return Y3, [engine.make_params(Y3, YumaConfig())] * N, W, S


@pytest.mark.parametrize("watch", [
    pytest.param([], id="empty"),
    pytest.param([8], id="index-M"),
    pytest.param([-1], id="negative"),
    pytest.param([0.5], id="float"),
    pytest.param([0, 3, 8], id="one-bad-of-three"),
    pytest.param([[0, 1]], id="two-dimensional"),
    pytest.param(torch.tensor([True, False]), id="bool-tensor"),
    pytest.param(np.array([0, 2 ** 40]), id="beyond-int32"),
])
def test_run_rejects_a_bad_watch_list_before_touching_the_device(no_device, watch):
    variant, params, W, S = run_args()
    with pytest.raises(ValueError, match="watch"):
        engine.run(variant, params, W, S, watch=watch)


def test_a_valid_watch_list_passes_validation():
    assert engine._watch_host([7, 0, 7], 8).tolist() == [7, 0, 7]
    assert engine._watch_host(torch.tensor([2], dtype=torch.int32), 3).tolist() == [2]
    assert engine._watch_host(np.array([1, 0], dtype=np.uint8), 2).tolist() == [1, 0]


def test_run_result_has_the_new_fields_with_defaults():
    r = engine.RunResult(None, None, None, None, None, {})
    assert r.B_watch is None and r.watch_cols is None and r.hist_epochs is None


def test_run_simulations_rejects_bad_columns_before_touching_the_device(no_device):
    case = builtin_cases[0]
    M = len(case.servers)
    runs = [SimulationRun(case, "Yuma 3 (Rhef)", YumaConfig())]
    with pytest.raises(ValueError, match="bonds_columns"):
        run_simulations(runs, bonds_columns=[M])
    with pytest.raises(ValueError, match="bonds_columns"):
        run_simulations(runs, bonds_columns=[])
    with pytest.raises(ValueError, match="bonds_columns"):
        run_simulations(runs, bonds_columns=[-1])
    with pytest.raises(ValueError, match="bonds_columns"):
        run_simulations(runs, bonds_columns=[0.5])
    # the message names the first run whose M is too small
    with pytest.raises(ValueError, match=r"run 0 .*M=" + str(M)):
        run_simulations(runs + runs, bonds_columns=[0, M])
