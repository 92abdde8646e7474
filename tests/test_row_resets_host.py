"""Validator-row events, host side (no GPU): the C-ABI of yuma_run_events and
its companions, yuma_events_native beside yuma_resets_native, the refusals that
come back before the first launch (equal from the direct run and the graph
form, in the order the header documents), the workspace of the row table, the
argument checks of engine.run(row_resets=) and
run_simulations(validator_resets=), which raise before anything touches a
device, and the register report of the 12 row-event scans."""

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
NEW_FUNCTIONS = ("yuma_run_events", "yuma_graph_create_events", "yuma_events_native", "yuma_workspace_bytes_events")
RUST, Y1, Y2, Y3, Y4 = range(5)
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4
MAXV = engine.MAX_VALIDATORS
ALWAYS = engine.RESET_ALWAYS


def header_code():
    text = open(os.path.join(ROOT, "include", "yuma_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def proto(name):
    return re.search(r"\b(\w+)\s+" + name + r"\s*\((.*?)\)\s*;", header_code(), flags=re.S)


def test_header_declares_the_entry_points_and_the_event_record():
    for name in NEW_FUNCTIONS[:3]:
        assert proto(name).group(1) == "int", name
    assert proto("yuma_workspace_bytes_events").group(1) == "size_t"
    for name in NEW_FUNCTIONS[:2]:
        args = re.sub(r"\s+", " ", proto(name).group(2))
        # yuma_run_resets's arguments with the row list and its length after n_events
        assert "int n_events, const yuma_row_event_t* row_events_dev, int n_row_events, void* workspace" in args
        resets = re.sub(r"\s+", " ", proto(name.replace("events", "resets")).group(2))
        assert args.replace("const yuma_row_event_t* row_events_dev, int n_row_events, ", "") == resets
    args = [re.sub(r"\s+", " ", a).strip() for a in proto("yuma_events_native").group(2).split(",")]
    assert args == ["int variant", "int N", "int E", "int V", "int M", "const yuma_outputs_t* out", "int flags"]
    body = re.search(r"typedef struct yuma_row_event \{([^}]*)\}\s*yuma_row_event_t;", header_code()).group(1)
    assert re.findall(r"\bint32_t\s+(\w+)\s*;", body) == [n for n, _ in engine.YumaRowEventC._fields_]
    assert [n for n, _ in engine.YumaRowEventC._fields_] == ["epoch", "scenario", "row", "reserved"]
    assert ctypes.sizeof(engine.YumaRowEventC) == 16


def test_library_exports_and_argtypes_match_the_header():
    lib = engine.load_library()
    for name in NEW_FUNCTIONS:
        assert name in engine.EXPORTED_SYMBOLS, name
        fn = getattr(lib, name)
        n_params = len([a for a in proto(name).group(2).split(",") if a.strip()])
        assert len(fn.argtypes) == n_params, name
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    a, b = list(lib.yuma_run_resets.argtypes), list(lib.yuma_run_events.argtypes)
    assert b == a[:13] + [vp, i32] + a[13:]
    a, b = list(lib.yuma_graph_create_resets.argtypes), list(lib.yuma_graph_create_events.argtypes)
    assert b == a[:14] + [vp, i32] + a[14:]
    assert list(lib.yuma_events_native.argtypes) == [i32] * 5 + [vp, i32]
    assert lib.yuma_events_native.restype is ctypes.c_int
    assert lib.yuma_workspace_bytes_events.restype is ctypes.c_size_t
    assert list(lib.yuma_workspace_bytes_events.argtypes) == list(lib.yuma_workspace_bytes.argtypes)
    # the records the issue leaves alone
    assert ctypes.sizeof(engine.YumaScanPlanC) == 80 and ctypes.sizeof(engine.YumaRunOptionsC) == 32
    assert ctypes.sizeof(engine.YumaResetEventC) == 16


@pytest.mark.parametrize("V,M", [(5, 8), (67, 12), (33, 68), (5, 1032), (MAXV, 8)])
def test_events_native_is_resets_native(V, M):
    """The grid of tests/test_resets_host.py's truth table: the same answer everywhere, both sides of each condition."""
    N, E = 2, 6
    seen = set()

    def same(*a, **kw):
        r = engine.events_native(*a, **kw)
        assert r == engine.resets_native(*a, **kw), (a, kw)
        seen.add(r)
        return r

    for variant in (Y3, Y4):
        assert same(variant, N, E, V, M) and same(variant, N, E, V, M, True)
        assert same(variant, N, E, V, M, want=("D", "R", "P", "T", "Sn", "bond_alpha", "alpha_ab"))
        assert not same(variant, N, E, V, M + 2)
        assert not same(variant, N, E, V, M, shared_inputs=True)
        assert not same(variant, N, E, V, M, w_u16=True)
        assert not same(variant, N, E, V, M, True, hist_bf16=True)
        for name in ("Wn", "Wc", "Wb", "B_inst", "Tv"):
            assert not same(variant, N, E, V, M, want=(name,)), name
        assert not same(variant, N, E, MAXV + 1, M)
        assert not same(variant, 0, E, V, M) and not same(variant, N, 0, V, M)
        assert not same(variant, N, E, 0, M) and not same(variant, N, E, V, 0)
    for variant in (RUST, Y1, Y2, 7, -1):
        assert not same(variant, N, E, V, M)
    assert seen == {True, False}


@pytest.mark.parametrize("variant,N,E,V,M", [(Y3, 2, 6, 5, 8), (Y4, 1, 5, 5, 1032), (Y3, 256, 100, 64, 4096), (Y1, 2, 3, 70, 10),
                                             (Y3, 4, 12, 5, 8), (Y3, 2, 6, 10, 8)])
def test_workspace_bytes_events(variant, N, E, V, M):
    lib = engine.load_library()
    for full in (0, 1):
        resets = lib.yuma_workspace_bytes_resets(variant, N, E, V, M, full)
        events = lib.yuma_workspace_bytes_events(variant, N, E, V, M, full)
        assert events == engine.workspace_bytes_events(variant, N, E, V, M, bool(full))
        table = events - resets
        assert table >= 4 * E * N * V        # one 32-bit word per (epoch, scenario, validator)
        assert table < 4 * E * N * V + 1024  # ... and padding only
    assert lib.yuma_workspace_bytes_events(variant, 0, E, V, M, 0) == 0


def test_the_row_table_grows_with_its_three_sizes():
    lib = engine.load_library()
    table = lambda N, E, V: (lib.yuma_workspace_bytes_events(Y3, N, E, V, 8, 0)
                             - lib.yuma_workspace_bytes_resets(Y3, N, E, V, 8, 0))
    base = table(4, 64, 16)
    assert table(8, 64, 16) == table(4, 128, 16) == table(4, 64, 32) == 2 * base == 2 * 4 * 4 * 64 * 16


# ---------------------------------------------------------------------------
# refusals before the first launch: no GPU, no HIP call. The pointers are never
# dereferenced (any non-null value stands for device memory).
# ---------------------------------------------------------------------------
P = 0x1000  # a non-null "device pointer"


def call_both(variant=Y3, N=2, E=6, V=5, M=8, events=P, n_events=3, rows=P, n_rows=2, ws_bytes=None, flags=0, hist=None,
              W=P, want=(), stride=1, out=True):
    """(code, text) of yuma_run_events and of yuma_graph_create_events."""
    lib = engine.load_library()
    outs = engine.YumaOutputsC(Dn=P, C=P, I=P, B_final=P, B_hist=hist, **{k: P for k in want})
    opts = engine.YumaRunOptionsC(flags=flags, hist_stride=stride, hist_first=0)
    if ws_bytes is None:
        ws_bytes = 1 << 40
    common = (variant, P, N, E, V, M, W, P, None, None, ctypes.addressof(outs) if out else None, events, n_events,
              rows, n_rows, P, ws_bytes, 0, ctypes.addressof(opts))
    rc_run = lib.yuma_run_events(*common, None, None)
    msg_run = lib.yuma_last_error().decode()
    h = ctypes.c_void_p()
    rc_graph = lib.yuma_graph_create_events(ctypes.byref(h), *common)
    msg_graph = lib.yuma_last_error().decode()
    assert h.value is None
    return (rc_run, msg_run), (rc_graph, msg_graph)


def ws(kind="events", variant=Y3, N=2, E=6, V=5, M=8):
    return getattr(engine.load_library(), "yuma_workspace_bytes" + {"plain": "", "resets": "_resets",
                                                                    "events": "_events"}[kind])(variant, N, E, V, M, 0)


@pytest.mark.parametrize("kw,code,text", [
    # 1. the options
    (dict(flags=64), EINVAL, "unknown run flags"),
    (dict(stride=-1, N=0), EINVAL, "hist_stride"),
    # 3. sizes
    (dict(N=0, W=None), EINVAL, "sizes must be positive"),
    (dict(V=MAXV + 1, W=None), EUNSUPPORTED, "YUMA_MAX_VALIDATORS"),
    # 4. NULL pointers, before the lists' own checks
    (dict(W=None, n_rows=-1), EINVAL, "null params"),
    (dict(out=False, rows=None), EINVAL, "null params"),
    # 5. the column list's checks, then n_row_events < 0, then n_row_events > 0 with a NULL list
    (dict(n_events=-1, n_rows=-1), EINVAL, "n_events=-1"),
    (dict(events=None, n_events=3, n_rows=-1), EINVAL, "NULL event list"),
    (dict(n_rows=-1), EINVAL, "n_row_events=-1"),
    (dict(n_rows=-1, rows=None, ws_bytes=16), EINVAL, "n_row_events=-1"),
    (dict(rows=None, n_rows=2), EINVAL, "NULL row event list"),
    (dict(rows=None, n_rows=2, ws_bytes=16, variant=Y1), EINVAL, "NULL row event list"),
    (dict(rows=None, n_rows=2, events=None, n_events=0), EINVAL, "NULL row event list"),
    # 6. the workspace size: yuma_workspace_bytes_resets is too small once there is a row list; one byte short
    (dict(ws_bytes=16), EWORKSPACE, "workspace"),
    (dict(ws_bytes=ws("plain")), EWORKSPACE, "workspace"),
    (dict(ws_bytes=ws("resets")), EWORKSPACE, "workspace"),
    (dict(ws_bytes=ws("events") - 1), EWORKSPACE, "workspace"),
    (dict(ws_bytes=ws("events") - 1, events=None, n_events=0), EWORKSPACE, "workspace"),
    (dict(ws_bytes=16, variant=Y1), EWORKSPACE, "workspace"),
    (dict(ws_bytes=16, M=10), EWORKSPACE, "workspace"),
    # 7. not native, then not in vector form: yuma_run_resets's refusals and text
    (dict(variant=RUST), EUNSUPPORTED, "yuma_resets_native"),
    (dict(variant=Y1), EUNSUPPORTED, "yuma_resets_native"),
    (dict(variant=Y2), EUNSUPPORTED, "yuma_resets_native"),
    (dict(M=10), EUNSUPPORTED, "yuma_resets_native"),
    (dict(flags=engine.RUN_SHARED_INPUTS), EUNSUPPORTED, "yuma_resets_native"),
    (dict(flags=engine.RUN_W_U16), EUNSUPPORTED, "yuma_resets_native"),
    (dict(flags=engine.RUN_HIST_BF16, hist=P), EUNSUPPORTED, "yuma_resets_native"),
    (dict(want=("Wn",)), EUNSUPPORTED, "yuma_resets_native"),
    (dict(want=("Tv",)), EUNSUPPORTED, "yuma_resets_native"),
    (dict(W=P + 4), EUNSUPPORTED, "need the vector form"),
    (dict(hist=P + 4), EUNSUPPORTED, "need the vector form"),
    (dict(events=None, n_events=0, variant=Y1), EUNSUPPORTED, "yuma_resets_native"),   # row events alone
    # 8. last: the row table's 32-bit epoch step
    (dict(N=1 << 19, V=1024, E=1, ws_bytes=1 << 62), EUNSUPPORTED, "2^29"),
    (dict(N=1 << 19, V=1024, E=1, ws_bytes=1 << 62, W=P + 4), EUNSUPPORTED, "need the vector form"),
    # an empty row list that is present (n_row_events = 0, a pointer) is a run with row events: the table's workspace
    (dict(n_rows=0, ws_bytes=ws("resets")), EWORKSPACE, "workspace"),
    (dict(n_rows=0, variant=Y1), EUNSUPPORTED, "yuma_resets_native"),
])
def test_refusals_without_a_gpu_are_equal_from_run_and_graph(kw, code, text):
    run, graph = call_both(**kw)
    assert run[0] == code and text in run[1], run
    assert graph == run


def test_the_exact_workspace_passes_the_size_check():
    """With yuma_workspace_bytes_events bytes the next refusal in the order is reached (here: not in vector form)."""
    run, graph = call_both(ws_bytes=ws("events"), W=P + 4)
    assert run[0] == EUNSUPPORTED and "need the vector form" in run[1] and graph == run


def test_no_row_events_is_yuma_run_resets():
    """n_row_events = 0 with a NULL list: yuma_run_resets's own checks, text and workspace size; with no column
    list either, yuma_run_opts's."""
    lib = engine.load_library()
    outs = engine.YumaOutputsC(Dn=P, C=P, I=P, B_final=P)
    opts = engine.YumaRunOptionsC()
    tail = (ctypes.addressof(opts), None, None)
    for variant, M, size, ev, n_ev in ((Y3, 8, ws("resets") - 1, P, 3), (Y1, 10, 1 << 40, P, 3), (Y3, 8, 16, P, 0),
                                       (Y3, 8, 1 << 40, None, 3), (Y3, 8, ws("plain") - 1, None, 0)):
        head = (variant, P, 2, 6, 5, M, P, P, None, None, ctypes.addressof(outs))
        rc = lib.yuma_run_events(*head, ev, n_ev, None, 0, P, size, 0, *tail)
        msg = lib.yuma_last_error().decode()
        rc2 = lib.yuma_run_resets(*head, ev, n_ev, P, size, 0, *tail)
        assert (rc, msg) == (rc2, lib.yuma_last_error().decode()) and rc < 0
        if ev is None and n_ev == 0:
            rc3 = lib.yuma_run_opts(*head, P, size, 0, *tail)
            assert (rc, msg) == (rc3, lib.yuma_last_error().decode())


def test_graph_handle_is_checked_after_the_options():
    lib = engine.load_library()
    outs = engine.YumaOutputsC(Dn=P, C=P, I=P, B_final=P)
    bad = engine.YumaRunOptionsC(flags=0, hist_stride=-1)
    args = (Y3, P, 0, 6, 5, 8, P, P, None, None, ctypes.addressof(outs), P, 3, P, 2, P, 1 << 40, 0)
    assert lib.yuma_graph_create_events(None, *args, ctypes.addressof(bad)) == EINVAL
    assert "hist_stride" in lib.yuma_last_error().decode()
    ok = engine.YumaRunOptionsC()
    assert lib.yuma_graph_create_events(None, *args, ctypes.addressof(ok)) == EINVAL
    assert "graph handle" in lib.yuma_last_error().decode()   # ... and before the sizes (N = 0)


# ---------------------------------------------------------------------------
# engine.run validates row_resets= on the host
# ---------------------------------------------------------------------------
@pytest.fixture()
def no_device(monkeypatch):
    """Any request for the device fails the test: validation comes first."""
    def boom():
        raise AssertionError("a device was asked for before the events were validated")
    monkeypatch.setattr(engine, "device", boom)


def run_args(variant=Y3, E=3, N=2, V=5, M=8):
    g = torch.Generator().manual_seed(1)
    W, S = torch.rand((E, N, V, M), generator=g), torch.rand((E, N, V), generator=g) + 0.5
    return variant, [engine.make_params(variant, YumaConfig())] * N, W, S


@pytest.mark.parametrize("bad,text", [
    ([(3, 0, 1)], "epoch 3"), ([(-1, 0, 1)], "epoch -1"),
    ([(1, 2, 1)], "scenario 2"), ([(1, -1, 1)], "scenario -1"),
    ([(1, 0, 5)], "validator 5"), ([(1, 0, -1)], "validator -1"),
    ([(1, 0, 1, 1)], "reserved 1"), ([(1, 0, 1, -1)], "reserved -1"),
    ([(0, 0, 0), (1, 1, 4), (1, 1, 9)], r"row_resets\[2\]"),
    ([(1, 0)], "shape"), ([1, 0, 1], "shape"), ([(1, 0, 1, 0, 0)], "shape"), ([(1.0, 0.0, 1.0)], "integers"),
    (torch.tensor([[1, 0, 5, 0]], dtype=torch.int32), "validator 5"),     # a CPU tensor is a host list
])
def test_run_rejects_bad_events_before_touching_the_device(no_device, bad, text):
    variant, params, W, S = run_args()
    with pytest.raises(ValueError, match=text):
        engine.run(variant, params, W, S, row_resets=bad)
    with pytest.raises(ValueError, match=text):
        engine.run(variant, params, W, S, row_resets=bad, resets=[(1, 0, 1, ALWAYS)])
    with pytest.raises(ValueError, match=text):
        engine.RunGraph(variant, params, W, S, row_resets=bad)


def test_host_events_accept_the_whole_range():
    ev = [(0, 0, 0), (2, 1, 4), (2, 1, 4), (1, 0, 3)]
    h = engine._row_resets_host(ev, 2, 3, 5)
    assert h.dtype == torch.int64 and h.tolist() == [list(e) + [0] for e in ev]
    assert engine._row_resets_host([], 2, 3, 5).shape == (0, 4)
    assert engine._row_resets_host(torch.tensor(ev, dtype=torch.int32), 2, 3, 5).tolist() == [list(e) + [0] for e in ev]
    assert engine._row_resets_host([e + (0,) for e in ev], 2, 3, 5).tolist() == [list(e) + [0] for e in ev]


@pytest.mark.parametrize("kw,text", [
    (dict(sched=[0, 1, 2]), "sched"), (dict(watch=[1]), "watch"), (dict(watch_rows=[1]), "watch_rows"),
    (dict(want_move=True), "want_move"), (dict(single_call=True), "single_call"),
    (dict(hist_dtype=torch.bfloat16, want_hist=True), "bfloat16"),
])
def test_run_rejects_the_combinations_before_touching_the_device(no_device, kw, text):
    variant, params, W, S = run_args()
    with pytest.raises(ValueError, match="row_resets= does not combine with .*" + text):
        engine.run(variant, params, W, S, row_resets=[(1, 0, 1)], **kw)


@pytest.mark.parametrize("variant", [RUST, Y1, Y2])
def test_run_rejects_the_other_variants_before_touching_the_device(no_device, variant):
    variant, params, W, S = run_args(variant)
    with pytest.raises(ValueError, match="Yuma 3 / Yuma 4"):
        engine.run(variant, params, W, S, row_resets=[(1, 0, 1)])
    with pytest.raises(ValueError, match="Yuma 3 / Yuma 4"):
        engine.run(variant, params, W, S, row_resets=[])


# ---------------------------------------------------------------------------
# run_simulations validates validator_resets on the host
# ---------------------------------------------------------------------------
def sim_runs(versions=("Yuma 3.1 (Rhef+reset)", "Yuma 4 (Rhef+relative bonds)")):
    case = builtin_cases[0]
    return [SimulationRun(case, v, YumaConfig()) for v in versions]


@pytest.mark.parametrize("bad,text", [
    ([None], "one entry"), ("ab", "one entry"), (3, "one entry"),
    ([[(1, 0, 0)], None], "pair"), ([[(1.0, 0)], None], "pair"), ([[(True, 0)], None], "pair"), ([[5], None], "pair"),
    ([[(-1, 0)], None], "negative"), ([None, [(1, -1)]], "index -1"), ([None, [(1, 10**6)]], "index 1000000"),
])
def test_run_simulations_rejects_bad_validator_resets_before_touching_the_device(no_device, bad, text):
    with pytest.raises(ValueError, match=text):
        run_simulations(sim_runs(), validator_resets=bad)


@pytest.mark.parametrize("version", ["Yuma 0 (subtensor)", "Yuma 1 (paper)", "Yuma 2 (Adrian-Fish)"])
def test_run_simulations_rejects_pairs_for_the_other_versions(no_device, version):
    runs = sim_runs(("Yuma 3 (Rhef)", version))
    with pytest.raises(ValueError, match="not Yuma 3.x / Yuma 4"):
        run_simulations(runs, validator_resets=[None, [(1, 0)]])


@pytest.mark.parametrize("kw,text", [
    (dict(dedup_inputs=True), "dedup_inputs"), (dict(bonds_columns=[0]), "bonds_columns"),
    (dict(bonds_validators=[0]), "bonds_validators"), (dict(bonds_movement=True), "bonds_movement"),
    (dict(bonds_dtype=torch.bfloat16), "bfloat16"),
])
def test_run_simulations_rejects_the_combinations_before_touching_the_device(no_device, kw, text):
    with pytest.raises(ValueError, match="validator_resets does not combine with .*" + text):
        run_simulations(sim_runs(), validator_resets=[[(1, 0)], None], **kw)


# ---------------------------------------------------------------------------
# the register report of the row-event kernels, from the built library's code object
# ---------------------------------------------------------------------------
def test_no_row_event_kernel_spills_or_uses_scratch():
    """The 12 RW forms of k_bonds_elem -- the twins of the 12 RL forms, read the
    way tests/test_resets_host.py reads those -- report no spilled VGPR, no
    spilled SGPR and no scratch, and take the RL forms' block with the second
    pointer appended."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kcompare

    meta = kcompare.kernels(engine.LIB_PATH)
    forms, rl = kcompare.elem_forms(meta, "RW"), set(kcompare.elem_forms(meta, "RL"))
    rw = {k: meta[k][2] for k in forms}
    assert len(rw) == 12 and len(rl) == 12, sorted(rw)
    assert {kcompare.with_form(k, "RW", "RL") for k in rw} == rl   # the twins, shape by shape
    assert sorted({variant for variant, _, _ in forms.values()}) == ["3", "4"]
    fields = dict(zip(kcompare.FIELDS, range(len(kcompare.FIELDS))))
    for name, m in rw.items():
        for f in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
            assert m[fields[f]] == "0", (name, f, m)
        assert m[fields["kernarg_segment_size"]] == "232", (name, m)   # the RL forms' 224 bytes and the row table pointer
