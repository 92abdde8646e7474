"""The C ABI's run and graph entry points against each other (gpu marker).

engine.run goes through yuma_run_request / yuma_graph_create_request only
(single_call: yuma_epoch), so every positional entry point -- yuma_run,
yuma_run_profiled, yuma_run_ex, yuma_run_opts, the seven feature rungs from
yuma_run_sched to yuma_run_events, and their yuma_graph_create_* twins -- is
called here through ctypes:

  * every entry point that can express a run gives the same bits: Dn, C, I,
    B_final and B_hist, each call into fresh sentinel-filled outputs;
  * a refused call is refused alike by a run entry point and its graph twin:
    the same code, the same yuma_last_error text, no graph handle, and not a
    byte of the outputs or the workspace written.

  * each feature rung gives the bits of yuma_run_request on the equivalent
    record, its own output (B_watch, B_move, B_rows, B_rowstat) included, and
    one rung of each branch (rows, events) those of yuma_graph_create_request.

One small vector-form case: N = 2, E = 5, V = 70, M = 260 (the 64-miner-tile
history scan, a partial last tile), chunk_epochs = 2, an fp32 history."""

from __future__ import annotations

import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from yuma_simulation._internal import engine, synth  # noqa: E402
from yuma_simulation._internal.yumas import SimulationHyperparameters, YumaConfig  # noqa: E402

Y1, Y3, Y4 = engine.VARIANT_YUMA1, engine.VARIANT_YUMA3, engine.VARIANT_YUMA4
N, E, V, M, CHUNK = 2, 5, 70, 260, 2
SENTINEL = -7.0
OUT_SHAPES = (("Dn", (E, N, V)), ("C", (E, N, M)), ("I", (E, N, M)), ("B_final", (N, V, M)), ("B_hist", (E, N, V, M)))
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4


def _params(variant, dev):
    """Two scenarios that differ (bond_penalty, kappa): a sweep's classes are not one."""
    cfgs = (YumaConfig(simulation=SimulationHyperparameters(bond_penalty=0.99)),
            YumaConfig(simulation=SimulationHyperparameters(bond_penalty=0.5, kappa=0.4)))
    plist = [engine.make_params(variant, c) for c in cfgs]
    return plist, engine.params_tensor(plist, dev)


class Call:
    """The arguments of one run in device memory, every output and the
    workspace filled with a sentinel."""

    def __init__(self, variant, prm, W, S, *, hist=True, hist_offset=0, short=0, K=None, nbytes=None):
        self.dev = dev = engine.device()
        self.lib = engine.load_library()
        self.variant, self.prm, self.W, self.S, self.K = variant, prm, W, S, K
        self.o = {k: torch.full(s, SENTINEL, dtype=torch.float32, device=dev)
                  for k, s in OUT_SHAPES if hist or k != "B_hist"}
        ptr = {k: t.data_ptr() for k, t in self.o.items()}
        if hist_offset:  # B_hist at a byte offset into a buffer with room for it
            self.o["B_hist"] = torch.full((E * N * V * M + 4,), SENTINEL, dtype=torch.float32, device=dev)
            ptr["B_hist"] = self.o["B_hist"].data_ptr() + hist_offset
        self.outs = engine.YumaOutputsC(**{k: ptr.get(k) for k in engine.OUTPUT_FIELDS})
        if nbytes is None:
            nbytes = (engine.workspace_bytes(variant, N, E, V, M, False) if K is None
                      else engine.workspace_bytes_sched(variant, N, E, K, V, M, False))
        self.ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=dev)
        self.ws_bytes = nbytes - short
        self.stream = torch.cuda.current_stream(dev).cuda_stream
        self.sched = None if K is None else torch.zeros(E, dtype=torch.int32, device=dev)

    @property
    def args(self):
        """variant ... chunk_epochs, as every run entry point takes them (with K and the schedule under one)."""
        a = (self.variant, self.prm.data_ptr(), N, E, V, M, self.W.data_ptr(), self.S.data_ptr(), None, None,
             ctypes.addressof(self.outs), self.ws.data_ptr(), self.ws_bytes, CHUNK)
        if self.K is not None:
            a = a[:4] + (self.K,) + a[4:8] + (self.sched.data_ptr(),) + a[8:]
        return a

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((t == SENTINEL).all()) for t in self.o.values()) and bool((self.ws == 0x5A).all())

    def result(self):
        torch.cuda.synchronize()
        assert not any(bool((t == SENTINEL).any()) for t in self.o.values())  # every element was written
        return self.o


def _direct(make, fn, *tail):
    """One run through the run entry point `fn` (tail: what follows chunk_epochs)."""
    c = make()
    rc = getattr(c.lib, fn)(*c.args, *[c.stream if t == "stream" else t for t in tail])
    assert rc == 0, (fn, rc, c.lib.yuma_last_error())
    return c.result()


def _graph(make, fn, *tail):
    """One launch of the graph that `fn` captures."""
    c = make()
    h = ctypes.c_void_p()
    torch.cuda.synchronize()
    rc = getattr(c.lib, fn)(ctypes.byref(h), *c.args, *tail)
    assert rc == 0 and h.value, (fn, rc, c.lib.yuma_last_error())
    try:
        assert c.untouched()  # a capture runs nothing
        assert c.lib.yuma_graph_launch(h, c.stream) == 0
        return c.result()
    finally:
        torch.cuda.synchronize()
        c.lib.yuma_graph_destroy(h)


def _assert_same(ref, got, what):
    for k, _ in OUT_SHAPES:
        assert torch.equal(ref[k], got[k]), (what, k)


def test_every_entry_point_gives_the_same_bits():
    dev = engine.device()
    _, prm = _params(Y3, dev)
    W = torch.from_numpy(synth.weights(0xE17, E, N, V, M)).to(dev)
    S = torch.from_numpy(synth.stakes(0xE17, E, N, V, period=3)).to(dev)
    make = lambda: Call(Y3, prm, W, S)  # noqa: E731
    zero = engine.YumaRunOptionsC()
    phases = (ctypes.c_float * len(engine.PHASES))()
    ref = _direct(make, "yuma_run", "stream")
    assert float(ref["B_hist"].abs().max()) > 0.0
    runs = {
        "yuma_run_profiled": _direct(make, "yuma_run_profiled", "stream", phases),
        "yuma_run_ex": _direct(make, "yuma_run_ex", 0, "stream", None),
        "yuma_run_opts NULL": _direct(make, "yuma_run_opts", None, "stream", None),
        "yuma_run_opts zeroed": _direct(make, "yuma_run_opts", ctypes.addressof(zero), "stream", None),
        "yuma_graph_create": _graph(make, "yuma_graph_create"),
        "yuma_graph_create_ex": _graph(make, "yuma_graph_create_ex", 0),
        "yuma_graph_create_opts": _graph(make, "yuma_graph_create_opts", None),
    }
    assert sum(phases) > 0.0
    for what, got in runs.items():
        _assert_same(ref, got, what)


def test_shared_inputs_through_the_flags_and_the_options_record():
    dev = engine.device()
    plist, prm = _params(Y4, dev)
    W = torch.from_numpy(synth.weights(0xE18, E, 1, V, M)).to(dev)
    S = torch.from_numpy(synth.stakes(0xE18, E, 1, V, period=3)).to(dev)
    make = lambda: Call(Y4, prm, W, S)  # noqa: E731
    sh = engine.RUN_SHARED_INPUTS
    opts = engine.YumaRunOptionsC(flags=sh)
    ref = _direct(make, "yuma_run_opts", ctypes.addressof(opts), "stream", None)
    _assert_same(ref, _direct(make, "yuma_run_ex", sh, "stream", None), "yuma_run_ex")
    _assert_same(ref, _graph(make, "yuma_graph_create_ex", sh), "yuma_graph_create_ex")
    _assert_same(ref, _graph(make, "yuma_graph_create_opts", ctypes.addressof(opts)), "yuma_graph_create_opts")
    res = engine.run(Y4, plist, W, S, want_hist=True, chunk_epochs=CHUNK, shared_inputs=True)
    torch.cuda.synchronize()
    got = {"Dn": res.Dn, "C": res.C, "I": res.I, "B_final": res.B_final, "B_hist": res.B_hist}
    _assert_same(ref, got, "engine.run(shared_inputs=True)")


def _refusal(variant, flags, *, hist=True, hist_offset=0, short=0, K=None):
    """(code, text) that the run entry point and its graph twin both return
    for one argument set; nothing written, no handle."""
    dev = engine.device()
    _, prm = _params(variant, dev)
    W = torch.ones((K or E, N, V, M), dtype=torch.float32, device=dev)
    S = torch.ones((K or E, N, V), dtype=torch.float32, device=dev)
    c = Call(variant, prm, W, S, hist=hist, hist_offset=hist_offset, short=short, K=K)
    opts = engine.YumaRunOptionsC(flags=flags)
    run_fn, graph_fn = ((c.lib.yuma_run_opts, c.lib.yuma_graph_create_opts) if K is None
                        else (c.lib.yuma_run_sched, c.lib.yuma_graph_create_sched))
    rc = run_fn(*c.args, ctypes.addressof(opts), c.stream, None)
    text = c.lib.yuma_last_error()
    h = ctypes.c_void_p()
    rcg = graph_fn(ctypes.byref(h), *c.args, ctypes.addressof(opts))
    textg = c.lib.yuma_last_error()
    assert not h.value
    assert (rc, text) == (rcg, textg)
    assert c.untouched()
    return rc, text


def test_run_and_graph_entry_points_refuse_alike():
    rc, text = _refusal(Y1, engine.RUN_W_U16)
    assert rc == EUNSUPPORTED and b"yuma_u16_native" in text
    rc, text = _refusal(Y3, engine.RUN_HIST_BF16, hist=False)
    assert rc == EINVAL and b"B_hist" in text
    # B_hist 4 bytes off: not the 8-byte alignment of a bfloat16 history (found before the capture opens:
    # the validation makes no HIP call)
    rc, text = _refusal(Y3, engine.RUN_HIST_BF16, hist_offset=4)
    assert rc == EUNSUPPORTED and b"B_hist 8-byte aligned" in text
    rc, text = _refusal(Y1, 0, K=2)
    assert rc == EUNSUPPORTED and b"yuma_sched_native" in text
    # two refusals at once: the workspace size comes first on both paths
    rc, text = _refusal(Y1, engine.RUN_W_U16, short=1)
    assert rc == EWORKSPACE and b"workspace" in text


# ---------------------------------------------------------------------------
# the feature rungs against yuma_run_request / yuma_graph_create_request
# ---------------------------------------------------------------------------
R = engine
SCHED = (0, 1, 1, 0, 1)
WATCH, ROWS = (3, 259, 0), (69, 0)
COL_EVENTS = ((2, 0, 5, R.RESET_ALWAYS), (3, 1, -1, R.RESET_ALWAYS), (1, 1, 7, R.RESET_IF_ZERO_CONSENSUS))
ROW_EVENTS = ((2, 1, 4, 0), (4, 0, 69, 0))


class RungCall(Call):
    """A Call with one feature rung's inputs and its own sentinel-filled output: `positional` is the rung's
    argument list up to chunk_epochs, `record` the equivalent yuma_request_t."""

    def __init__(self, rung, variant, prm, W, S):
        dev = engine.device()
        lib = engine.load_library()
        size = (variant, N, E, V, M, 0)
        nbytes = {"rowstat": lib.yuma_workspace_bytes_rowstat, "resets": lib.yuma_workspace_bytes_resets,
                  "events": lib.yuma_workspace_bytes_events}.get(rung)
        K = len(set(SCHED)) if rung == "sched" else None
        super().__init__(variant, prm, W[:K] if K else W, S[:K] if K else S, hist=rung not in ("move", "rowstat"), K=K,
                         nbytes=None if nbytes is None else int(nbytes(*size)))
        self.rung = rung
        i32 = lambda rows: torch.tensor(rows, dtype=torch.int32, device=dev)  # noqa: E731
        own = lambda *shape: torch.full(shape, SENTINEL, dtype=torch.float32, device=dev)  # noqa: E731
        if K:
            self.sched.copy_(i32(SCHED))
        self.lists = {"watch": i32(WATCH), "rows": i32(ROWS), "resets": i32(COL_EVENTS), "events": i32(ROW_EVENTS)}
        own_shape = {"watch": (E, N, V, len(WATCH)), "move": (E, N, 2), "rows": (E, N, len(ROWS), M),
                     "rowstat": (E, N, V, 3)}.get(rung)
        if own_shape is not None:
            self.o["B_" + rung] = own(*own_shape)

    def _own(self):
        return self.o["B_" + self.rung].data_ptr()

    @property
    def positional(self):
        a = self.args
        if self.rung in ("sched", "resets", "events"):
            ev = (self.lists["resets"].data_ptr(), len(COL_EVENTS))
            rev = (self.lists["events"].data_ptr(), len(ROW_EVENTS))
            ins = {"sched": (), "resets": ev, "events": ev + rev}[self.rung]
            k = 11 if self.rung != "sched" else len(a) - 3
            return a[:k] + ins + a[k:]
        a = a[:4] + (0,) + a[4:8] + (None,) + a[8:]  # no schedule: K = 0, NULL
        none = (None, 0, None)
        ins = {"watch": (self.lists["watch"].data_ptr(), len(WATCH), self._own()),
               "move": none + (self._own(),),
               "rows": none + (None, self.lists["rows"].data_ptr(), len(ROWS), self._own()),
               "rowstat": none + (None,) + none + (self._own(),)}[self.rung]
        return a[:13] + ins + a[13:]

    @property
    def record(self):
        req = R.YumaRequestC(struct_size=ctypes.sizeof(R.YumaRequestC), variant=self.variant, N=N, E=E, K=self.K or 0, V=V,
                             M=M, params_dev=self.prm.data_ptr(), W=self.W.data_ptr(), S=self.S.data_ptr(),
                             sched_dev=None if self.K is None else self.sched.data_ptr(),
                             out=ctypes.addressof(self.outs), workspace=self.ws.data_ptr(),
                             workspace_bytes=self.ws_bytes, chunk_epochs=CHUNK)
        if self.rung == "watch":
            req.sections, req.watch_dev, req.n_watch, req.B_watch = (
                R.REQ_WATCH, self.lists["watch"].data_ptr(), len(WATCH), self._own())
        elif self.rung == "move":
            req.sections, req.B_move = R.REQ_MOVE, self._own()
        elif self.rung == "rows":
            req.sections, req.rows_dev, req.n_rows, req.B_rows = (
                R.REQ_ROWS, self.lists["rows"].data_ptr(), len(ROWS), self._own())
        elif self.rung == "rowstat":
            req.sections, req.B_rowstat = R.REQ_ROWSTAT, self._own()
        if self.rung in ("resets", "events"):
            req.sections, req.events_dev, req.n_events = R.REQ_RESETS, self.lists["resets"].data_ptr(), len(COL_EVENTS)
        if self.rung == "events":
            req.sections |= R.REQ_ROW_EVENTS
            req.row_events_dev, req.n_row_events = self.lists["events"].data_ptr(), len(ROW_EVENTS)
        return req


def _rung_inputs(dev):
    _, prm = _params(Y3, dev)
    W = torch.from_numpy(synth.weights(0xE19, E, N, V, M)).to(dev)
    S = torch.from_numpy(synth.stakes(0xE19, E, N, V, period=3)).to(dev)
    return prm, W, S


def _same_outputs(ref, got, what):
    assert ref.keys() == got.keys(), what
    for k in ref:
        assert torch.equal(ref[k].view(torch.int32), got[k].view(torch.int32)), (what, k)


@pytest.mark.parametrize("rung", ["sched", "watch", "move", "rows", "rowstat", "resets", "events"])
def test_a_rung_and_its_request_give_the_same_bits(rung):
    dev = engine.device()
    prm, W, S = _rung_inputs(dev)
    c = RungCall(rung, Y3, prm, W, S)
    rc = getattr(c.lib, "yuma_run_" + rung)(*c.positional, None, c.stream, None)
    assert rc == 0, (rung, rc, c.lib.yuma_last_error())
    ref = c.result()
    c = RungCall(rung, Y3, prm, W, S)
    req = c.record
    assert int(c.lib.yuma_workspace_bytes_request(ctypes.addressof(req))) == c.ws_bytes
    rc = c.lib.yuma_run_request(ctypes.addressof(req), c.stream, None)
    assert rc == 0, (rung, rc, c.lib.yuma_last_error())
    _same_outputs(ref, c.result(), "yuma_run_request")
    if rung in ("resets", "events"):  # the events did something: the plain run differs
        plain = _direct(lambda: Call(Y3, prm, W, S), "yuma_run", "stream")
        assert not torch.equal(plain["B_final"], ref["B_final"])
    if rung not in ("rows", "events"):
        return
    c = RungCall(rung, Y3, prm, W, S)
    req = c.record
    h = ctypes.c_void_p()
    torch.cuda.synchronize()
    rc = c.lib.yuma_graph_create_request(ctypes.byref(h), ctypes.addressof(req))
    assert rc == 0 and h.value, (rung, rc, c.lib.yuma_last_error())
    try:
        assert c.untouched()  # a capture runs nothing
        assert c.lib.yuma_graph_launch(h, c.stream) == 0
        _same_outputs(ref, c.result(), "yuma_graph_create_request")
    finally:
        torch.cuda.synchronize()
        c.lib.yuma_graph_destroy(h)


def test_a_refused_request_is_refused_alike_by_run_and_graph():
    """Yuma 1 takes no watch list: the same code and text from both, no handle, nothing written."""
    dev = engine.device()
    _, prm = _params(Y1, dev)
    W = torch.ones((E, N, V, M), dtype=torch.float32, device=dev)
    S = torch.ones((E, N, V), dtype=torch.float32, device=dev)
    c = RungCall("watch", Y1, prm, W, S)
    req = c.record
    rc = c.lib.yuma_run_request(ctypes.addressof(req), c.stream, None)
    text = c.lib.yuma_last_error()
    h = ctypes.c_void_p()
    rcg = c.lib.yuma_graph_create_request(ctypes.byref(h), ctypes.addressof(req))
    assert not h.value and (rc, text) == (rcg, c.lib.yuma_last_error())
    assert rc == EUNSUPPORTED and b"yuma_watch_native" in text
    assert c.untouched()
