"""Validator-row events (gpu marker): engine.run(..., row_resets=),
RunGraph(..., row_resets=) and run_simulations(..., validator_resets=).

The reference is the definition: the chain of plain engine.run calls (no
resets=, no row_resets=) cut at the distinct event epochs, each on W[a:b],
S[a:b] from the carried B_final whose rows and columns torch has zeroed
(chain() below); it never runs the code under test. Every comparison is bit
equality of Dn, C, I, B_final and every history slot. Inputs follow
tests/test_gpu_resets.py. The shapes are its six: the smallest that cross each
boundary of the four scans the events are native in; G below is the distance
between a lane's two rows where the scan gives a lane two (plan.rows == 2)."""

from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import yuma_oracle as orc  # noqa: E402
from yuma_simulation._internal import engine, simulation_utils, synth  # noqa: E402
from yuma_simulation._internal.cases import cases as builtin_cases  # noqa: E402
from yuma_simulation._internal.simulation_utils import SimulationRun, run_simulations  # noqa: E402
from yuma_simulation._internal.yumas import (  # noqa: E402
    SimulationHyperparameters,
    YumaConfig,
    YumaParams,
)

Y3, Y4 = engine.VARIANT_YUMA3, engine.VARIANT_YUMA4
ALWAYS, IF_ZERO = engine.RESET_ALWAYS, engine.RESET_IF_ZERO_CONSENSUS
GROUP = [pytest.param(Y3, False, id="yuma3"), pytest.param(Y4, False, id="yuma4"),
         pytest.param(Y4, True, id="yuma4-liquid")]
NAMES = ("Dn", "C", "I", "B_final")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "gpu tests need a ROCm GPU"
    engine.load_library()
    yield
    torch.cuda.empty_cache()


def bits(t):
    return engine._int_view(t.contiguous())


def config(liquid=False, i=0):
    """Scenario i's configuration: no two scenarios hold the same bonds."""
    return YumaConfig(simulation=SimulationHyperparameters(kappa=0.5 + 0.05 * (i % 2), bond_penalty=0.99),
                      yuma_params=YumaParams(bond_alpha=0.1 + 0.07 * (i % 8), liquid_alpha=liquid,
                                             decay_rate=0.1 + 0.03 * (i % 8), capacity_alpha=0.1 + 0.02 * (i % 8)))


def params(variant, liquid, N, **kw):
    return [engine.make_params(variant, config(liquid, i), **kw) for i in range(N)]


def inputs(E, N, V, M, seed=0, zero_col=None):
    """tests/test_gpu_resets.py's recipe: W [E,N,V,M], S [E,N,V]; a fifth of
    the weights exact zeros, validator 1's weights all zero, the last validator
    without stake. zero_col = (epoch, column): that column's consensus is
    exactly 0 at that epoch."""
    g = torch.Generator().manual_seed(1000 * V + M + seed)
    W = torch.rand((E, N, V, M), generator=g)
    W[torch.rand((E, N, V, M), generator=g) < 0.2] = 0.0
    W[:, :, 1 % V, :] = 0.0
    S = torch.rand((E, N, V), generator=g) + 0.25
    S[:, :, V - 1] = 0.0
    if zero_col is not None:
        e = zero_col[0]
        W[e] = 0.5 + 0.5 * torch.rand((N, V, M), generator=g)
        W[e, :, 1 % V, :] = 0.0
        W[e, :, :, zero_col[1]] = 0.0
    return W, S


def chain(variant, prm, W, S, B_init, rows, cols=(), *, want_hist=False, **kw):
    """The definition: plain runs cut at the distinct event epochs. rows:
    in-range (epoch, scenario, validator) tuples; cols: in-range (epoch,
    scenario, column, mode) tuples. Returns a dict of Dn, C, I, B_final and the
    dense B_hist (want_hist)."""
    E = W.shape[0]
    by = {}
    for t, n, v in rows:
        by.setdefault(t, ([], []))[0].append((n, v))
    for t, n, c, mode in cols:
        by.setdefault(t, ([], []))[1].append((n, c, mode))

    def zero(B, evs, prevC):
        B = B.clone()
        for n, v in evs[0]:
            B[n, v, :] = 0.0
        for n, c, mode in evs[1]:
            if mode == ALWAYS and c == -1:
                B[n] = 0.0
            elif c >= 0 and (mode == ALWAYS or (prevC is not None and float(prevC[n, c]) == 0.0)):
                B[n, :, c] = 0.0
        return B

    B = None if B_init is None else B_init.to(engine.device(), torch.float32)
    if B is not None and 0 in by:
        B = zero(B, by[0], None)
    cuts = [0] + sorted(t for t in by if 0 < t < E) + [E]
    parts, last = [], None
    for a, b in zip(cuts[:-1], cuts[1:]):
        if a > 0:
            B = zero(last.B_final, by[a], last.C[-1])
        last = engine.run(variant, prm, W[a:b], S[a:b], B, want_hist=want_hist, **kw)
        assert "resets_path" not in last.extra  # the plain path: the reference never runs the code under test
        parts.append(last)
    out = {k: torch.cat([getattr(p, k) for p in parts]) for k in ("Dn", "C", "I")}
    out["B_final"] = last.B_final
    if want_hist:
        out["B_hist"] = torch.cat([p.B_hist for p in parts])
    torch.cuda.synchronize()
    return out


def assert_equal(got, want, what=""):
    for k in NAMES:
        assert torch.equal(bits(getattr(got, k)), bits(want[k])), (what, k)
    if "B_hist" in want:
        slots = list(got.hist_epochs)
        assert got.B_hist.shape[0] == len(slots)
        assert torch.equal(bits(got.B_hist), bits(want["B_hist"][slots])), (what, "B_hist")


def check(variant, prm, W, S, rows, B_init=None, *, cols=None, path="native", want_hist=False, chain_cols=None,
          chain_prm=None, **kw):
    """run(row_resets=rows[, resets=cols]) against the chain; returns (the run, the chain)."""
    ref_kw = {k: v for k, v in kw.items() if k in ("shared_inputs",)}
    ref = chain(variant, prm if chain_prm is None else chain_prm, W, S, B_init, rows,
                (cols or ()) if chain_cols is None else chain_cols, want_hist=want_hist, **ref_kw)
    extra = {} if cols is None else {"resets": cols}
    got = engine.run(variant, prm, W, S, B_init, row_resets=rows, want_hist=want_hist, **extra, **kw)
    torch.cuda.synchronize()
    assert got.extra["resets_path"] == path
    assert_equal(got, ref)
    return got, ref


def row_events(E, V, n, G):
    """Row events of scenario n: row 0, row V - 1 (a part-filled row block),
    where a lane owns two rows (G: their distance) a row of the second set and
    its neighbour, the same row in consecutive epochs, an event at epoch 0 and
    at the last epoch, duplicates."""
    t2 = min(2, E - 1)
    ev = [(1, n, 0), (t2, n, V - 1), (0, n, 0), (E - 1, n, 0), (E - 1, n, min(2, V - 1))]
    if G:
        ev += [(t2, n, G), (1, n, min(G + 1, V - 1))]
    ev += [(t, n, min(3, V - 1)) for t in range(1, E)]
    return ev + ev[:2] + [(E - 1, n, V - 1)] * 2


def out_of_range(E, N, V, n):
    return [(E, n, 0, 0), (-1, n, 0, 0), (1, N, 0, 0), (1, -1, 0, 0), (1, n, V, 0), (1, n, -1, 0), (1, n, 1, 1),
            (1, n, 1, -1), (2**31 - 1, n, 0, 0), (1, 2**31 - 1, 0, 0), (1, n, 2**31 - 1, 0)]


SHAPES = [
    pytest.param(6, 2, 5, 260, False, ("flat1", 2, 2), 0, id="flat1-2x2-blocks"),
    pytest.param(4, 64, 512, 8, False, ("flat2", 64, 1), 4, id="flat2"),
    pytest.param(6, 2, 33, 68, True, ("tile_hist", 2, 2), 16, id="tile_hist-2x2-blocks"),
    pytest.param(5, 1, 5, 1032, True, ("wide", 2, 2), 2, id="wide-2x2-blocks"),
    pytest.param(3, 1, 1030, 8, False, ("flat1", 258, 1), 0, id="above-1024-validators"),
    pytest.param(3, 1, 1030, 8, True, ("tile_hist", 33, 1), 16, id="above-1024-validators-history"),
]


@pytest.mark.parametrize("variant,liquid", GROUP)
@pytest.mark.parametrize("E,N,V,M,hist,shape,G", SHAPES)
def test_shapes(variant, liquid, E, N, V, M, hist, shape, G):
    plan = engine.scan_plan(variant, N, E, V, M, hist)
    assert plan.form == "k_bonds_elem" and (plan.shape, plan.rowblocks, plan.cblocks) == shape, plan
    assert plan.rows == (2 if G else 1), plan
    assert engine.events_native(variant, N, E, V, M, hist)
    n = N - 1
    W, S = inputs(E, N, V, M)
    prm = params(variant, liquid, N)
    ev = row_events(E, V, n, G)
    plain = engine.run(variant, prm, W, S, want_hist=hist)
    got, ref = check(variant, prm, W, S, ev, want_hist=hist)
    assert got.extra["row_resets"].dtype == torch.int32 and tuple(got.extra["row_resets"].shape) == (len(ev), 4)
    # the comparison is not of equal zeros: the events changed scenario n, and no other
    assert not torch.equal(bits(got.B_final[n]), bits(plain.B_final[n]))
    assert not torch.equal(bits(got.Dn[:, n]), bits(plain.Dn[:, n]))
    for k in NAMES[:3]:
        assert torch.equal(bits(getattr(got, k)[:, :n]), bits(getattr(plain, k)[:, :n])), k
    assert torch.equal(bits(got.B_final[:n]), bits(plain.B_final[:n]))
    if hist:
        assert torch.equal(bits(got.B_hist[:, :n]), bits(plain.B_hist[:, :n]))
    # out-of-range and reserved != 0 events, passed unchecked as a device tensor, change nothing
    dev = torch.tensor([e + (0,) for e in ev] + out_of_range(E, N, V, n), dtype=torch.int32, device=engine.device())
    assert_equal(engine.run(variant, prm, W, S, row_resets=dev, want_hist=hist), ref, "with out-of-range events")
    # nor do duplicates
    once = sorted(set(ev))
    assert len(once) < len(ev)
    assert_equal(engine.run(variant, prm, W, S, row_resets=once, want_hist=hist), ref, "without the duplicates")
    # an [n, 3] device tensor
    dev3 = torch.tensor(ev, dtype=torch.int32, device=engine.device())
    assert_equal(engine.run(variant, prm, W, S, row_resets=dev3, want_hist=hist), ref, "[n, 3]")


@pytest.mark.parametrize("variant,liquid", GROUP)
@pytest.mark.parametrize("E,N,V,M,hist,G", [(6, 2, 33, 68, True, 16), (6, 2, 5, 260, False, 0), (4, 3, 9, 8, False, 4)],
                         ids=["tile_hist", "flat1", "flat1-small"])
def test_events_at_epoch_0(variant, liquid, E, N, V, M, hist, G):
    n = N - 1
    W, S = inputs(E, N, V, M)
    prm = params(variant, liquid, N)
    ev = row_events(E, V, n, G)
    g = torch.Generator().manual_seed(7)
    B0 = torch.rand((N, V, M), generator=g) * (2.0 ** 58 if variant == Y3 else 0.5)
    # with a B_init they fire ...
    with_init, _ = check(variant, prm, W, S, ev, B0, want_hist=hist)
    no_e0 = engine.run(variant, prm, W, S, B0, row_resets=[e for e in ev if e[0] != 0], want_hist=hist)
    torch.cuda.synchronize()
    assert not torch.equal(bits(with_init.Dn[0, n]), bits(no_e0.Dn[0, n]))
    if hist:  # ... and the history's slot 0 shows it, in row 0 alone
        assert not torch.equal(bits(with_init.B_hist[0, n, 0]), bits(no_e0.B_hist[0, n, 0]))
        assert torch.equal(bits(with_init.B_hist[0, n, 1:]), bits(no_e0.B_hist[0, n, 1:]))
    # without a B_init they do nothing
    a = engine.run(variant, prm, W, S, row_resets=ev, want_hist=hist)
    b = engine.run(variant, prm, W, S, row_resets=[e for e in ev if e[0] != 0], want_hist=hist)
    for k in NAMES:
        assert torch.equal(bits(getattr(a, k)), bits(getattr(b, k))), k
    only0 = engine.run(variant, prm, W, S, row_resets=[(0, n, v) for v in range(V)], want_hist=hist)
    plain = engine.run(variant, prm, W, S, want_hist=hist)
    for k in NAMES:
        assert torch.equal(bits(getattr(only0, k)), bits(getattr(plain, k))), k


@pytest.mark.parametrize("variant,liquid", GROUP)
def test_every_row_position(variant, liquid):
    """Every one of the 33 rows of scenario 1 has an event, at a different epoch from its neighbours."""
    E, N, V, M = 6, 2, 33, 68
    W, S = inputs(E, N, V, M)
    prm = params(variant, liquid, N)
    ev = [(1 + v % (E - 1), 1, v) for v in range(V)]
    plan = engine.scan_plan(variant, N, E, V, M, True)
    assert (plan.shape, plan.rowblocks, plan.cblocks, plan.rows) == ("tile_hist", 2, 2, 2), plan
    got, ref = check(variant, prm, W, S, ev, want_hist=True)
    plain = engine.run(variant, prm, W, S, want_hist=True)
    assert torch.equal(bits(got.B_hist[:, 0]), bits(plain.B_hist[:, 0]))
    assert not torch.equal(bits(got.B_final[1]), bits(plain.B_final[1]))
    check(variant, prm, W, S, ev)  # the history-less scan (flat1) on the same events


@pytest.mark.parametrize("variant,liquid", GROUP)
@pytest.mark.parametrize("E,N,V,M,hist,G", [(6, 2, 33, 68, True, 16), (5, 1, 5, 1032, True, 2), (6, 2, 33, 68, False, 0)],
                         ids=["tile_hist", "wide", "no-history"])
def test_strided_and_absent_history(variant, liquid, E, N, V, M, hist, G):
    W, S = inputs(E, N, V, M)
    prm = params(variant, liquid, N)
    ev = row_events(E, V, N - 1, G)
    if hist:
        got, _ = check(variant, prm, W, S, ev, want_hist=True, hist_stride=2, hist_first=1)
        assert got.hist_epochs == tuple(range(1, E, 2))
        plan = engine.scan_plan(variant, N, E, V, M, True, hist_stride=2, hist_first=1)
        assert plan.hs and plan.shape in ("tile_hist", "wide")
    else:
        got, _ = check(variant, prm, W, S, ev)
        assert got.B_hist is None


@pytest.mark.parametrize("variant,liquid", GROUP)
@pytest.mark.parametrize("hist", [False, True], ids=["flat1", "tile_hist"])
def test_event_at_a_chunks_first_epoch(variant, liquid, hist):
    E, N, V, M = 6, 2, 5, 68
    W, S = inputs(E, N, V, M, zero_col=(1, 7))
    prm = params(variant, liquid, N)
    rows = [(2, 1, 0), (2, 1, 4), (4, 0, 2), (3, 1, 3)]
    cols = [(2, 1, 7, IF_ZERO), (4, 1, 66, ALWAYS)]
    _, ref = check(variant, prm, W, S, rows, cols=cols, want_hist=hist)
    for chunk in (1, 2, 0):
        got = engine.run(variant, prm, W, S, row_resets=rows, resets=cols, want_hist=hist, chunk_epochs=chunk)
        torch.cuda.synchronize()
        assert got.extra["resets_path"] == "native"
        assert_equal(got, ref, f"chunk_epochs={chunk}")


@pytest.mark.parametrize("variant,liquid,mode", [pytest.param(Y3, False, ALWAYS, id="yuma31"),
                                                 pytest.param(Y4, False, IF_ZERO, id="yuma4"),
                                                 pytest.param(Y4, True, IF_ZERO, id="yuma4-liquid")])
@pytest.mark.parametrize("hist", [False, True], ids=["flat1", "tile_hist"])
def test_rows_beside_columns_and_the_params_own_reset(variant, liquid, mode, hist):
    """Row events, column events (unconditional, a conditional one that fires and one that does not) and the
    scenario's own reset, all at epoch 3."""
    E, N, V, M = 6, 2, 5, 68
    W, S = inputs(E, N, V, M, zero_col=(2, 5))
    own = params(variant, liquid, N, reset_mode=mode, reset_epoch=3, reset_index=5, n_miners=M, n_epochs=E)
    plain = params(variant, liquid, N)
    rows = [(3, 1, 0), (3, 1, 4), (3, 0, 2), (1, 1, 1)]
    cols = [(3, 1, 66, ALWAYS), (3, 1, 5, IF_ZERO), (3, 0, 9, IF_ZERO), (3, 0, 6, ALWAYS), (4, 1, 0, ALWAYS)]
    folded = cols + [(3, n, 5, mode) for n in range(N)]
    got, ref = check(variant, own, W, S, rows, cols=cols, want_hist=hist, chain_cols=folded, chain_prm=plain)
    assert got.extra["resets"] is not None and got.extra["row_resets"] is not None
    # each kind did something
    no_rows = engine.run(variant, own, W, S, resets=cols, want_hist=hist)
    no_cols = engine.run(variant, own, W, S, row_resets=rows, want_hist=hist)
    no_own = engine.run(variant, plain, W, S, row_resets=rows, resets=cols, want_hist=hist)
    for other in (no_rows, no_cols, no_own):
        assert not torch.equal(bits(other.B_final), bits(got.B_final))


@pytest.mark.parametrize("variant,liquid", GROUP)
def test_empty_lists(variant, liquid):
    E, N, V, M = 6, 2, 5, 260
    W, S = inputs(E, N, V, M)
    prm = params(variant, liquid, N)
    cols = [(1, 1, 0, ALWAYS), (4, 0, 259, ALWAYS)]
    with_cols = engine.run(variant, prm, W, S, resets=cols)
    got = engine.run(variant, prm, W, S, resets=cols, row_resets=[])
    assert got.extra["resets_path"] == "native" and tuple(got.extra["row_resets"].shape) == (0, 4)
    plain = engine.run(variant, prm, W, S)
    both = engine.run(variant, prm, W, S, resets=[], row_resets=[])
    only = engine.run(variant, prm, W, S, row_resets=torch.zeros((0, 3), dtype=torch.int32, device=engine.device()))
    torch.cuda.synchronize()
    assert not torch.equal(bits(with_cols.B_final), bits(plain.B_final))
    for k in NAMES:
        assert torch.equal(bits(getattr(got, k)), bits(getattr(with_cols, k))), k
        assert torch.equal(bits(getattr(both, k)), bits(getattr(plain, k))), k
        assert torch.equal(bits(getattr(only, k)), bits(getattr(plain, k))), k


# ---------------------------------------------------------------------------
# graphs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant,liquid", GROUP)
@pytest.mark.parametrize("E,N,V,M,hist", [(6, 2, 5, 260, False), (6, 2, 33, 68, True)], ids=["flat1", "tile_hist"])
def test_graph_replays_and_rereads_the_list(variant, liquid, E, N, V, M, hist):
    W, S = inputs(E, N, V, M)
    prm = params(variant, liquid, N)
    dev = engine.device()
    first = [(1, 1, 0, 0), (4, 1, V - 1, 0), (2, 0, 2, 0), (E, 0, 0, 0), (3, 1, 1, 7)]
    second = [(5, 0, 3, 0), (2, 1, V - 1, 0), (2, 1, V - 1, 0), (1, 1, 4, 0), (3, 0, 0, 0)]
    cols = [(2, 1, 3, ALWAYS)]
    lst = torch.tensor(first, dtype=torch.int32, device=dev)
    d0 = engine.run(variant, prm, W, S, row_resets=[e[:3] for e in first[:3]], resets=cols, want_hist=hist)
    d1 = engine.run(variant, prm, W, S, row_resets=[e[:3] for e in second], resets=cols, want_hist=hist)
    assert not torch.equal(bits(d0.B_final), bits(d1.B_final))
    g = engine.RunGraph(variant, prm, W, S, row_resets=lst, resets=cols, want_hist=hist)
    try:
        assert g.result.extra["resets_path"] == "native" and g.result.extra["row_resets"] is lst
        for want in (d0, d0, d1):
            if want is d1:
                lst.copy_(torch.tensor(second, dtype=torch.int32))  # rewritten in place between two replays
            r = g.launch()
            torch.cuda.synchronize()
            for k in NAMES:
                assert torch.equal(bits(getattr(r, k)), bits(getattr(want, k))), k
            if hist:
                assert torch.equal(bits(r.B_hist), bits(want.B_hist))
    finally:
        g.close()


# ---------------------------------------------------------------------------
# fallbacks: the chain itself
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant,liquid", GROUP)
@pytest.mark.parametrize("hist", [False, True], ids=["no-history", "history"])
def test_the_scalar_form_takes_the_segments(variant, liquid, hist):
    E, N, V, M = 6, 2, 9, 10  # M % 4 != 0
    W, S = inputs(E, N, V, M, zero_col=(3, 7))
    prm = params(variant, liquid, N)
    rows = [(1, 1, 8), (4, 1, 0), (4, 0, 3), (5, 0, 3), (1, 1, 8), (0, 0, 0)]
    cols = [(4, 1, 7, IF_ZERO), (2, 0, 9, ALWAYS)]
    assert not engine.events_native(variant, N, E, V, M, hist)
    kw = dict(hist_stride=2, hist_first=1) if hist else {}
    got, _ = check(variant, prm, W, S, rows, cols=cols, path="segments", want_hist=hist, **kw)
    assert got.extra["row_resets"] is None
    plain = engine.run(variant, prm, W, S)
    assert not torch.equal(bits(got.B_final), bits(plain.B_final))
    check(variant, prm, W, S, rows, path="segments", want_hist=hist, **kw)  # row events alone
    # a device list is read back for the chain; what the device code would ignore is ignored here too
    dev = torch.tensor([r + (0,) for r in rows] + out_of_range(E, N, V, 1), dtype=torch.int32, device=engine.device())
    again = engine.run(variant, prm, W, S, row_resets=dev, resets=cols, want_hist=hist, **kw)
    assert again.extra["resets_path"] == "segments"
    for k in NAMES:
        assert torch.equal(bits(getattr(again, k)), bits(getattr(got, k))), k
    with pytest.raises(engine.EngineError, match="resets"):
        engine.RunGraph(variant, prm, W, S, row_resets=rows, want_hist=hist)


def test_shared_inputs_take_the_segments():
    E, V, M = 6, 6, 8
    W, S = inputs(E, 1, V, M)
    prm = params(Y3, False, 3)
    rows = [(1, 1, 0), (4, 2, 5), (2, 0, 3), (5, 1, 3)]
    got, _ = check(Y3, prm, W, S, rows, path="segments", want_hist=True, shared_inputs=True)
    plain = engine.run(Y3, prm, W, S, shared_inputs=True)
    assert not torch.equal(bits(got.B_final), bits(plain.B_final))
    with pytest.raises(engine.EngineError, match="resets"):
        engine.RunGraph(Y3, prm, W, S, row_resets=rows, shared_inputs=True)


@pytest.mark.parametrize("variant,liquid", GROUP)
@pytest.mark.parametrize("V", [5, 8])
def test_uint16_weights_take_the_segments(variant, liquid, V):
    E, N, M = 6, 2, 68
    g = torch.Generator().manual_seed(11)
    W = torch.randint(0, 65536, (E, N, V, M), generator=g, dtype=torch.int32).to(torch.uint16)
    _, S = inputs(E, N, V, M)
    prm = params(variant, liquid, N)
    rows = [(1, 1, 0), (4, 1, V - 1), (2, 0, 2), (3, 1, 3)]
    got, _ = check(variant, prm, W, S, rows, path="segments", want_hist=True)
    assert got.extra["w_path"] == "u16"
    with pytest.raises(engine.EngineError, match="resets"):
        engine.RunGraph(variant, prm, W, S, row_resets=rows)


# ---------------------------------------------------------------------------
# the oracle, and the public surface
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant,name", [(Y3, orc.YUMA3), (Y4, orc.YUMA4)], ids=["yuma3", "yuma4"])
def test_oracle_with_the_rows_zeroed_by_hand(variant, name):
    E, N, V, M = 5, 2, 32, 200
    W, S = synth.weights(0x5EED5, E, N, V, M), synth.stakes(0x5EED5, E, N, V, period=2)
    cfgs = [YumaConfig(yuma_params=YumaParams(bond_alpha=0.1 + 0.07 * i, decay_rate=0.1 + 0.03 * i,
                                              capacity_alpha=0.1 + 0.02 * i)) for i in range(N)]
    ev = [(1, 1, 0), (2, 0, 31), (2, 1, 16), (3, 1, 0), (4, 0, 3), (4, 1, 17), (0, 0, 1), (2, 0, 31)]
    got = engine.run(variant, [engine.make_params(variant, c) for c in cfgs], torch.from_numpy(W), torch.from_numpy(S),
                     row_resets=ev, want_hist=True)
    torch.cuda.synchronize()
    assert got.extra["resets_path"] == "native"
    for n in range(N):
        B = None
        for t in range(E):
            for te, ne, v in ev:
                if te == t and ne == n and B is not None:
                    B = B.copy()
                    B[v, :] = 0.0
            res = orc.epoch(name, W[t, n], S[t, n], B, cfgs[n])
            B = res["validator_bonds"]
            np.testing.assert_array_equal(got.C[t, n].cpu().numpy(), res["server_consensus_weight"])
            np.testing.assert_allclose(got.Dn[t, n].cpu().numpy(), res["validator_reward_normalized"], rtol=1e-5, atol=1e-7)
            np.testing.assert_allclose(got.B_hist[t, n].cpu().numpy(), B, rtol=1e-5, atol=1e-6 * float(np.abs(B).max()))


def test_run_simulations_validator_resets():
    versions = ("Yuma 3.1 (Rhef+reset)", "Yuma 4 (Rhef+relative bonds)")
    two = [c for c in builtin_cases if c.reset_bonds_epoch is None][:2]
    assert len(two) == 2
    runs = [SimulationRun(case, v, YumaConfig()) for case in two for v in versions]
    E0, V0, _ = two[0].packed_inputs()[0].shape
    pairs = [[(3, 0), (5, V0 - 1), (5, 1), (8, 0), (8, 0), (E0 + 40, 1)], [(2, 1), (3, 0)], None, [(1, 0), (6, 2 % V0)]]
    cols = [[(4, 0)], None, None, [(6, 1)]]
    ref = run_simulations(runs)
    got = run_simulations(runs, validator_resets=pairs, bond_resets=cols, bonds_every=2)
    changed = []
    for k, (run, (div, bonds, inc)) in enumerate(zip(runs, got)):
        case = run.case
        W, S = case.packed_inputs()
        E, V, M = W.shape
        variant, mode = simulation_utils.resolve_version(run.yuma_version)
        rows = [(e, 0, v) for e, v in (pairs[k] or ()) if e < E]
        cev = [(e, 0, i, mode) for e, i in (cols[k] or ()) if e < E] if mode != engine.RESET_NONE else []
        prm = [engine.make_params(variant, run.yuma_config)]
        c = chain(variant, prm, W[:, None], S[:, None], None, rows, cev, want_hist=True)
        slots = engine.hist_epochs(E, 2)
        assert len(bonds) == len(slots) and len(inc) == E
        assert all(torch.equal(bits(b), bits(c["B_hist"][t, 0].cpu())) for t, b in zip(slots, bonds))
        assert all(torch.equal(bits(x), bits(c["I"][t, 0].cpu())) for t, x in enumerate(inc))
        assert div == simulation_utils._dividends_per_1000_tao(case, run.yuma_config, S, c["Dn"][:, 0].cpu())
        changed.append(div != ref[k][0])
    assert any(changed) and not changed[2]  # (run 2 has no events)
