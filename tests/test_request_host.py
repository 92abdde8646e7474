"""The run request record, host side (no GPU): yuma_request_t's layout and its
own refusals, every positional rung against yuma_run_request /
yuma_graph_create_request on the equivalent record (the rungs' own refusal
tables, imported from their host test modules: the same code and
yuma_last_error text four ways), the section rules, the combinations no rung
could express, and yuma_workspace_bytes_request against the five positional
workspace functions. Nothing here touches a device: every refusal comes back
before the first launch, and the pointers are never dereferenced."""

from __future__ import annotations

import ctypes
import inspect
import itertools

import pytest

import test_move_host
import test_resets_host
import test_row_resets_host
import test_rows_host
import test_rowstat_host
import test_watch_host
from yuma_simulation._internal import engine

RUST, Y1, Y2, Y3, Y4 = range(5)
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4
P = 0x1000  # a non-null "device pointer"
R = engine
LISTS = ("watch", "n_watch", "b_watch", "b_move", "rows", "n_rows", "b_rows", "b_rowstat")


def given(bit, *args):
    """A rung's optional list is present when any of its arguments is given."""
    return bit if any(a not in (None, 0) for a in args) else 0


# Each rung's section mask, as include/yuma_hip.h states it beside the prototype.
MASKS = {
    "sched": lambda a: 0,
    "watch": lambda a: R.REQ_WATCH,
    "move": lambda a: R.REQ_MOVE | given(R.REQ_WATCH, a["watch"], a["n_watch"], a["b_watch"]),
    "rows": lambda a: (R.REQ_ROWS | given(R.REQ_WATCH, a["watch"], a["n_watch"], a["b_watch"])
                       | given(R.REQ_MOVE, a["b_move"])),
    "rowstat": lambda a: (R.REQ_ROWSTAT | given(R.REQ_WATCH, a["watch"], a["n_watch"], a["b_watch"])
                          | given(R.REQ_MOVE, a["b_move"]) | given(R.REQ_ROWS, a["rows"], a["n_rows"], a["b_rows"])),
    "resets": lambda a: given(R.REQ_RESETS, a["events"], a["n_events"]),
    "events": lambda a: (given(R.REQ_RESETS, a["events"], a["n_events"])
                         | given(R.REQ_ROW_EVENTS, a["row_events"], a["n_row_events"])),
}


def request_both(sections, *, variant=Y3, N=2, E=6, K=0, V=5, M=8, sched=None, watch=None, n_watch=0, b_watch=None,
                 b_move=None, rows=None, n_rows=0, b_rows=None, b_rowstat=None, events=None, n_events=0,
                 row_events=None, n_row_events=0, ws_bytes=None, flags=0, hist=None, W=P, want=(), stride=1, out=True,
                 struct_size=None, reserved=None):
    """(code, text) of yuma_run_request and of yuma_graph_create_request on one record."""
    lib = engine.load_library()
    outs = engine.YumaOutputsC(Dn=P, C=P, I=P, B_final=P, B_hist=hist, **{k: P for k in want})
    opts = engine.YumaRunOptionsC(flags=flags, hist_stride=stride, hist_first=0)
    req = engine.YumaRequestC(
        struct_size=ctypes.sizeof(engine.YumaRequestC) if struct_size is None else struct_size, sections=sections,
        variant=variant, N=N, E=E, K=K, V=V, M=M, params_dev=P, W=W, S=P, sched_dev=sched,
        out=ctypes.addressof(outs) if out else None, workspace=P, workspace_bytes=1 << 40 if ws_bytes is None else ws_bytes,
        opts=ctypes.addressof(opts), watch_dev=watch, n_watch=n_watch, B_watch=b_watch, B_move=b_move, rows_dev=rows,
        n_rows=n_rows, B_rows=b_rows, B_rowstat=b_rowstat, events_dev=events, n_events=n_events,
        row_events_dev=row_events, n_row_events=n_row_events)
    if reserved is not None:
        req.reserved[reserved] = 1
    rc_run = lib.yuma_run_request(ctypes.addressof(req), None, None)
    msg_run = lib.yuma_last_error().decode()
    h = ctypes.c_void_p()
    rc_graph = lib.yuma_graph_create_request(ctypes.byref(h), ctypes.addressof(req))
    msg_graph = lib.yuma_last_error().decode()
    assert h.value is None
    return (rc_run, msg_run), (rc_graph, msg_graph)


def table(module):
    """The parametrisation of a host module's refusal test: its (kw, code, text) rows."""
    mark, = [m for m in module.test_refusals_without_a_gpu_are_equal_from_run_and_graph.pytestmark
             if m.name == "parametrize"]
    return mark.args[1]


def rung_cases(rung, module):
    return [pytest.param(rung, module, row[0], id=f"{rung}-{i}") for i, row in enumerate(table(module))]


# ---------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------
def test_layout_is_the_librarys():
    """256 bytes (the library's static_assert pins the same number): a record of that size reaches the workspace
    refusal, which comes after everything the record itself can be refused for; any other size does not."""
    size = ctypes.sizeof(engine.YumaRequestC)
    assert size == 256
    assert engine.YumaRequestC.chunk_epochs.offset == 176 and engine.YumaRequestC.reserved.offset == 196
    run, graph = request_both(0, ws_bytes=16)
    assert run[0] == EWORKSPACE and "workspace 16 <" in run[1] and graph == run
    run, graph = request_both(R.REQ_WATCH | R.REQ_ROWS | R.REQ_MOVE, watch=P, n_watch=3, b_watch=P, b_move=P, rows=P,
                              n_rows=2, b_rows=P, sched=P, K=2, ws_bytes=16)
    assert run[0] == EWORKSPACE and graph == run
    for bad in (0, size - 8, size + 8):
        run, graph = request_both(0, struct_size=bad, ws_bytes=16)
        assert run[0] == EINVAL and "struct_size" in run[1] and graph == run


def test_reserved_words_unknown_sections_and_a_null_request_are_refused():
    for word in (0, 7, 14):
        run, graph = request_both(0, reserved=word)
        assert run[0] == EINVAL and "reserved must be 0" in run[1] and graph == run
    run, graph = request_both(64)
    assert run[0] == EINVAL and "unknown request sections" in run[1] and graph == run
    lib = engine.load_library()
    assert lib.yuma_run_request(None, None, None) == EINVAL
    h = ctypes.c_void_p()
    assert lib.yuma_graph_create_request(ctypes.byref(h), None) == EINVAL and h.value is None
    assert lib.yuma_workspace_bytes_request(None) == 0


def test_the_records_own_refusals_come_before_the_graph_handle():
    lib = engine.load_library()
    req = engine.YumaRequestC(struct_size=8)
    assert lib.yuma_graph_create_request(None, ctypes.addressof(req)) == EINVAL
    assert "struct_size" in lib.yuma_last_error().decode()
    req = engine.YumaRequestC(struct_size=ctypes.sizeof(engine.YumaRequestC))
    assert lib.yuma_graph_create_request(None, ctypes.addressof(req)) == EINVAL
    assert "graph handle" in lib.yuma_last_error().decode()


# ---------------------------------------------------------------------------
# shim equivalence: the rungs' refusal tables through the rung and through the record
# ---------------------------------------------------------------------------
def record_args(rung, module, kw):
    """The rung's call_both arguments (its defaults, then kw) as request_both's, with the rung's mask."""
    a = {k: p.default for k, p in inspect.signature(module.call_both).parameters.items()}
    a.update(kw)
    if rung == "events":  # (test_row_resets_host calls the row event list rows / n_rows)
        a["row_events"], a["n_row_events"] = a.pop("rows"), a.pop("n_rows")
    return MASKS[rung]({k: a.get(k) for k in LISTS + ("events", "n_events", "row_events", "n_row_events")}), a


@pytest.mark.parametrize("rung,module,kw", (
    rung_cases("watch", test_watch_host) + rung_cases("move", test_move_host) + rung_cases("rows", test_rows_host)
    + rung_cases("rowstat", test_rowstat_host) + rung_cases("resets", test_resets_host)
    + rung_cases("events", test_row_resets_host)))
def test_a_rung_and_its_record_refuse_alike(rung, module, kw):
    run, graph = module.call_both(**kw)
    assert run[0] != 0
    sections, a = record_args(rung, module, kw)
    req_run, req_graph = request_both(sections, **a)
    assert run == graph == req_run == req_graph


def sched_both(variant=Y3, N=2, E=6, K=2, V=5, M=8, sched=P, ws_bytes=1 << 40, flags=0, W=P, want=(), stride=1):
    """(code, text) of yuma_run_sched and of yuma_graph_create_sched."""
    lib = engine.load_library()
    outs = engine.YumaOutputsC(Dn=P, C=P, I=P, B_final=P, **{k: P for k in want})
    opts = engine.YumaRunOptionsC(flags=flags, hist_stride=stride, hist_first=0)
    common = (variant, P, N, E, K, V, M, W, P, sched, None, None, ctypes.addressof(outs), P, ws_bytes, 0,
              ctypes.addressof(opts))
    rc_run = lib.yuma_run_sched(*common, None, None)
    msg_run = lib.yuma_last_error().decode()
    h = ctypes.c_void_p()
    rc_graph = lib.yuma_graph_create_sched(ctypes.byref(h), *common)
    msg_graph = lib.yuma_last_error().decode()
    assert h.value is None
    return (rc_run, msg_run), (rc_graph, msg_graph)


# (test_sched_host.py has no refusal table of the C entry points: the rows are stated here, in run_plan's order)
@pytest.mark.parametrize("kw,code,text", [
    (dict(stride=-1), EINVAL, "hist_stride"),
    (dict(stride=-1, N=0), EINVAL, "hist_stride"),
    (dict(N=0), EINVAL, "sizes must be positive"),
    (dict(V=engine.MAX_VALIDATORS + 1), EUNSUPPORTED, "YUMA_MAX_VALIDATORS"),
    (dict(W=None), EINVAL, "null params"),
    (dict(ws_bytes=16), EWORKSPACE, "workspace"),
    (dict(ws_bytes=16, variant=Y1), EWORKSPACE, "workspace"),
    (dict(variant=Y1), EUNSUPPORTED, "yuma_sched_native"),
    (dict(M=10), EUNSUPPORTED, "yuma_sched_native"),
    (dict(want=("P",)), EUNSUPPORTED, "yuma_sched_native"),
    (dict(flags=engine.RUN_SHARED_INPUTS), EUNSUPPORTED, "yuma_sched_native"),
    (dict(W=P + 4), EUNSUPPORTED, "needs the vector form"),
    (dict(flags=engine.RUN_HIST_BF16), EINVAL, "YUMA_RUN_HIST_BF16 without out->B_hist"),
    (dict(flags=engine.RUN_W_U16, want=("Wn",)), EUNSUPPORTED, "yuma_sched_native"),
])
def test_the_sched_rung_and_its_record_refuse_alike(kw, code, text):
    run, graph = sched_both(**kw)
    assert run[0] == code and text in run[1], run
    a = dict(K=2, sched=P)
    a.update(kw)
    assert run == graph == request_both(0, **a)[0] == request_both(0, **a)[1]


def test_the_sched_rungs_own_early_check_stays_the_rungs():
    """yuma_run_sched's schedule is mandatory and checked before the sizes; the record's is optional, and run_plan
    refuses K without a pointer after them."""
    run, graph = sched_both(sched=None, N=0)
    assert run == graph and run[0] == EINVAL and "the schedule pointer is NULL" in run[1]
    run, graph = sched_both(K=0, N=0)
    assert run == graph and run[0] == EINVAL and "K=0 stored slices" in run[1]
    run, graph = request_both(0, K=2, sched=None, N=0)
    assert run == graph and run[0] == EINVAL and "sizes must be positive" in run[1]
    run, graph = request_both(0, K=2, sched=None)
    assert run == graph and run[0] == EINVAL and "K=2 stored slices without a schedule pointer" in run[1]
    run, graph = request_both(0, K=0, sched=P)
    assert run == graph and run[0] == EINVAL and "K=0 stored slices" in run[1]


# ---------------------------------------------------------------------------
# section rules
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kw,text", [
    (dict(watch=P), "without YUMA_REQ_WATCH"),
    (dict(n_watch=3), "without YUMA_REQ_WATCH"),
    (dict(b_watch=P), "without YUMA_REQ_WATCH"),
    (dict(b_move=P), "without YUMA_REQ_MOVE"),
    (dict(rows=P), "without YUMA_REQ_ROWS"),
    (dict(n_rows=2), "without YUMA_REQ_ROWS"),
    (dict(b_rows=P), "without YUMA_REQ_ROWS"),
    (dict(b_rowstat=P), "without YUMA_REQ_ROWSTAT"),
    (dict(events=P), "without YUMA_REQ_RESETS"),
    (dict(n_events=1), "without YUMA_REQ_RESETS"),
    (dict(row_events=P), "without YUMA_REQ_ROW_EVENTS"),
    (dict(n_row_events=1), "without YUMA_REQ_ROW_EVENTS"),
])
def test_a_field_of_an_absent_section_is_refused(kw, text):
    run, graph = request_both(0, **kw)
    assert run[0] == EINVAL and text in run[1] and graph == run
    # ... after the options, before the sizes
    assert request_both(0, N=0, **kw)[0] == run
    assert "hist_stride" in request_both(0, stride=-1, **kw)[0][1]


def test_the_bit_states_how_a_null_is_read():
    """yuma_run_move refuses a NULL B_move where yuma_run_rows reads it as "no movement": with the record the first
    is YUMA_REQ_MOVE with a NULL field, the second a clear bit. Likewise the empty watch and row lists."""
    rows = dict(rows=P, n_rows=2, b_rows=P)
    run, graph = request_both(R.REQ_ROWS | R.REQ_MOVE, ws_bytes=16, **rows)
    assert run[0] == EINVAL and "B_move is NULL" in run[1] and graph == run
    assert run == test_move_host.call_both(b_move=None, ws_bytes=16)[0]
    run, graph = request_both(R.REQ_ROWS, ws_bytes=16, **rows)
    assert run[0] == EWORKSPACE and graph == run
    assert run == test_rows_host.call_both(b_move=None, n_rows=2, ws_bytes=16)[0]
    # the watch list: mandatory to yuma_run_watch, optional to yuma_run_move
    run, _ = request_both(R.REQ_WATCH)
    assert run[0] == EINVAL and run == test_watch_host.call_both(watch=None, n_watch=0, b_watch=None)[0]
    assert request_both(R.REQ_MOVE, b_move=P, ws_bytes=16)[0][0] == EWORKSPACE
    # the row list: mandatory to yuma_run_rows, optional to yuma_run_rowstat
    run, _ = request_both(R.REQ_ROWS)
    assert run[0] == EINVAL and "n_rows=0" in run[1]
    assert run == test_rows_host.call_both(rows=None, n_rows=0, b_rows=None)[0]
    assert request_both(R.REQ_ROWSTAT, b_rowstat=P, ws_bytes=16)[0][0] == EWORKSPACE
    # a present event section with an empty list is refused as the rung refuses n > 0 with NULL; present and
    # empty is the scan with the tables (its workspace)
    run, _ = request_both(R.REQ_RESETS, n_events=2)
    assert run[0] == EINVAL and "NULL event list" in run[1]
    plain = engine.workspace_bytes(Y3, 2, 6, 5, 8, False)
    assert request_both(R.REQ_RESETS, ws_bytes=plain)[0][0] == EWORKSPACE


# ---------------------------------------------------------------------------
# combinations no positional rung could express
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("events", [
    dict(sections=R.REQ_RESETS, events=P, n_events=3),
    dict(sections=R.REQ_ROW_EVENTS, row_events=P, n_row_events=2),
    dict(sections=R.REQ_RESETS | R.REQ_ROW_EVENTS, events=P, n_events=3, row_events=P, n_row_events=2),
])
@pytest.mark.parametrize("other", [
    dict(sections=0, sched=P, K=2),
    dict(sections=R.REQ_WATCH, watch=P, n_watch=3, b_watch=P),
    dict(sections=R.REQ_MOVE, b_move=P),
    dict(sections=R.REQ_ROWS, rows=P, n_rows=2, b_rows=P),
    dict(sections=R.REQ_ROWSTAT, b_rowstat=P),
], ids=["sched", "watch", "move", "rows", "rowstat"])
def test_events_beside_another_section_are_unsupported(events, other):
    kw = {**events, **other}
    kw.pop("sections")
    run, graph = request_both(events["sections"] | other["sections"], **kw)
    assert run[0] == EUNSUPPORTED and "reset events do not combine" in run[1], run
    assert graph == run
    # the workspace size is still refused first, and the record's own errors before that
    assert request_both(events["sections"] | other["sections"], ws_bytes=16, **kw)[0][0] == EWORKSPACE


# ---------------------------------------------------------------------------
# workspace
# ---------------------------------------------------------------------------
def ws_request(sections, variant, N, E, K, V, M, full):
    outs = engine.YumaOutputsC(Tv=P if full else None)
    req = engine.YumaRequestC(struct_size=ctypes.sizeof(engine.YumaRequestC), sections=sections, variant=variant, N=N,
                              E=E, K=K, V=V, M=M, out=ctypes.addressof(outs))
    return int(engine.load_library().yuma_workspace_bytes_request(ctypes.addressof(req)))


def test_workspace_bytes_request_is_each_positional_function():
    lib = engine.load_library()
    for variant, V, M, E, K, full in itertools.product(range(5), (5, 70, 1030), (6, 8, 260), (1, 6), (0, 3), (0, 1)):
        N = 2
        a = (variant, N, E, V, M, full)
        if K:
            want = {0: int(lib.yuma_workspace_bytes_sched(variant, N, E, K, V, M, full))}
        else:
            want = {0: int(lib.yuma_workspace_bytes(*a)),
                    R.REQ_ROWSTAT: int(lib.yuma_workspace_bytes_rowstat(*a)),
                    R.REQ_RESETS: int(lib.yuma_workspace_bytes_resets(*a)),
                    R.REQ_ROW_EVENTS: int(lib.yuma_workspace_bytes_events(*a)),
                    R.REQ_RESETS | R.REQ_ROW_EVENTS: int(lib.yuma_workspace_bytes_events(*a))}
        for sections, nbytes in want.items():
            assert nbytes > 0 and ws_request(sections, variant, N, E, K, V, M, full) == nbytes, (a, K, sections)
        # the lists and B_move need no workspace of their own
        assert ws_request(R.REQ_WATCH | R.REQ_MOVE | R.REQ_ROWS, variant, N, E, K, V, M, full) == want[0]
    for bad in (dict(N=0), dict(E=0), dict(V=-1), dict(M=0), dict(K=-1)):
        a = dict(variant=Y3, N=2, E=6, K=0, V=5, M=8, full=0)
        a.update(bad)
        for sections in (0, R.REQ_ROWSTAT, R.REQ_RESETS, R.REQ_ROW_EVENTS):
            assert ws_request(sections, **a) == 0, (bad, sections)
    # out may be NULL: validator_trust not requested
    req = engine.YumaRequestC(struct_size=ctypes.sizeof(engine.YumaRequestC), variant=Y3, N=2, E=6, V=5, M=8)
    assert int(lib.yuma_workspace_bytes_request(ctypes.addressof(req))) == engine.workspace_bytes(Y3, 2, 6, 5, 8, False)
    req.struct_size = 8
    assert int(lib.yuma_workspace_bytes_request(ctypes.addressof(req))) == 0


def test_engine_types_the_positional_rungs_from_one_table():
    """load_library's table gives the lists the header's prototypes have (their host tests pin each splice): here
    only the lengths, and the three request entry points."""
    lib = engine.load_library()
    for name, n in (("sched", 19), ("watch", 22), ("move", 23), ("rows", 26), ("rowstat", 27), ("resets", 19),
                    ("events", 21)):
        assert len(getattr(lib, "yuma_run_" + name).argtypes) == n, name
        assert len(getattr(lib, "yuma_graph_create_" + name).argtypes) == n - 1, name
    assert len(lib.yuma_run_request.argtypes) == 3 and len(lib.yuma_graph_create_request.argtypes) == 2
    assert lib.yuma_workspace_bytes_request.restype is ctypes.c_size_t
    for name in ("yuma_run_request", "yuma_graph_create_request", "yuma_workspace_bytes_request"):
        assert name in engine.EXPORTED_SYMBOLS
