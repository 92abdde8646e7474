"""Bond reset events (gpu marker): engine.run(..., resets=), RunGraph(...,
resets=) and run_simulations(..., bond_resets=).

The reference is the definition: the chain of existing runs cut at the distinct
event epochs, each on W[a:b], S[a:b] from the carried B_final whose columns
torch has zeroed (chain() below, written on engine.run without resets=). Every
comparison is bit equality of Dn, C, I, B_final and every history slot. Inputs
follow tests/test_gpu_move.py: random weights with planted exact zeros, an
all-zero weight row, a zero-stake validator, and zero_col / full_col to make a
conditional event fire or not. The shapes are the smallest that cross each
boundary of the four scans the events are native in."""

from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import yuma_oracle as orc  # noqa: E402
from yuma_simulation._internal import engine, simulation_utils, synth  # noqa: E402
from yuma_simulation._internal.cases import LAST, BaseCase  # noqa: E402
from yuma_simulation._internal.simulation_utils import SimulationRun, run_simulations  # noqa: E402
from yuma_simulation._internal.yumas import (  # noqa: E402
    SimulationHyperparameters,
    YumaConfig,
    YumaParams,
)

Y1, Y3, Y4 = engine.VARIANT_YUMA1, engine.VARIANT_YUMA3, engine.VARIANT_YUMA4
ALWAYS, IF_ZERO = engine.RESET_ALWAYS, engine.RESET_IF_ZERO_CONSENSUS
GROUP = [pytest.param(Y3, False, id="yuma3"), pytest.param(Y4, True, id="yuma4-liquid")]
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


def inputs(E, N, V, M, seed=0, zero_col=None, full_col=None):
    """tests/test_gpu_move.py's recipe: W [E,N,V,M], S [E,N,V]; a fifth of the
    weights exact zeros, validator 1's weights all zero, the last validator
    without stake. zero_col = (epoch, column): that column's consensus is
    exactly 0 at that epoch; full_col = (epoch, column): it is not."""
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
    if full_col is not None:
        W[full_col[0], :, :, full_col[1]] = 0.5
    return W, S


def chain(variant, prm, W, S, B_init, events, *, want_hist=False, **kw):
    """The definition: runs without resets=, cut at the distinct event epochs.
    events: in-range (epoch, scenario, column, mode) tuples. Returns a dict of
    Dn, C, I, B_final and the dense B_hist (want_hist)."""
    E = W.shape[0]
    by = {}
    for t, n, c, mode in events:
        by.setdefault(t, []).append((n, c, mode))

    def zero(B, evs, prevC):
        B = B.clone()
        for n, c, mode in evs:
            if mode == ALWAYS and c == -1:
                B[n] = 0.0
            elif mode == ALWAYS or (mode == IF_ZERO and c >= 0 and prevC is not None and float(prevC[n, c]) == 0.0):
                if c >= 0:
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


def check(variant, prm, W, S, events, B_init=None, *, path="native", want_hist=False, shape=None, chain_events=None,
          chain_prm=None, **kw):
    """run(resets=events) against the chain on the in-range events; returns (the run, the chain)."""
    ref_kw = {k: v for k, v in kw.items() if k in ("shared_inputs",)}
    ref = chain(variant, prm if chain_prm is None else chain_prm, W, S, B_init,
                events if chain_events is None else chain_events, want_hist=want_hist, **ref_kw)
    got = engine.run(variant, prm, W, S, B_init, resets=events, want_hist=want_hist, **kw)
    torch.cuda.synchronize()
    assert got.extra["resets_path"] == path
    assert_equal(got, ref)
    if shape is not None:
        E, N, V, M = W.shape
        plan = engine.scan_plan(variant, N, E, V, M, want_hist, hist_stride=kw.get("hist_stride", 1),
                                hist_first=kw.get("hist_first"))
        assert plan.form == "k_bonds_elem" and (plan.shape, plan.rowblocks, plan.cblocks) == shape, plan
    return got, ref


def event_list(E, M, n, t_cond, zc, fc):
    """Events of scenario n: the quad's first and last lanes, the 64 / 256 /
    1024 boundaries and M - 1; every column in one epoch; column -1; the same
    column in consecutive epochs; duplicates; epoch 0; a conditional event that
    fires (zc) and one that does not (fc) at t_cond; and one at the last epoch."""
    cols = sorted({0, 3, 4, M - 1, M - 4} | {c for c in (63, 64, 255, 256, 1023, 1024) if c < M})
    ev = [(1, n, c, ALWAYS) for c in cols]
    ev += [(0, n, 3, ALWAYS), (0, n, zc, IF_ZERO)]                 # (a conditional event never fires at epoch 0)
    ev += [(t_cond, n, zc, IF_ZERO), (t_cond, n, fc, IF_ZERO)]
    if E > 3:
        # (both before the epoch that plants the conditional events' consensus: a column zeroed there stays zero)
        ev += [(min(2, t_cond - 2), n, c, ALWAYS) for c in range(M)]   # every column, one event each
        t_all = min(3, t_cond - 2)
        ev += [(t_all, n, -1, ALWAYS), (t_all, n, -1, IF_ZERO)]    # every column at once; the conditional form is ignored
    ev += [(t, n, 3, ALWAYS) for t in range(1, E)]                 # the same column in consecutive epochs
    ev += ev[:3] + [(E - 1, n, M - 1, ALWAYS)] * 2                 # duplicates
    return ev


def out_of_range(E, N, M, n):
    return [(E, n, 0, ALWAYS), (-1, n, 0, ALWAYS), (1, N, 0, ALWAYS), (1, -1, 0, ALWAYS), (1, n, M, ALWAYS),
            (1, n, -2, ALWAYS), (1, n, 0, 0), (1, n, 0, 3), (1, n, 0, -1), (2**31 - 1, n, 0, ALWAYS)]


SHAPES = [
    pytest.param(6, 2, 5, 260, False, ("flat1", 2, 2), id="flat1-2x2-blocks"),
    pytest.param(4, 64, 512, 8, False, ("flat2", 64, 1), id="flat2"),
    pytest.param(6, 2, 33, 68, True, ("tile_hist", 2, 2), id="tile_hist-2x2-blocks"),
    pytest.param(5, 1, 5, 1032, True, ("wide", 2, 2), id="wide-2x2-blocks"),
    pytest.param(3, 1, 1030, 8, False, ("flat1", 258, 1), id="above-1024-validators"),
    pytest.param(3, 1, 1030, 8, True, ("tile_hist", 33, 1), id="above-1024-validators-history"),
]


@pytest.mark.parametrize("variant,liquid", GROUP)
@pytest.mark.parametrize("E,N,V,M,hist,shape", SHAPES)
def test_shapes(variant, liquid, E, N, V, M, hist, shape):
    n, t = N - 1, E - 1
    zc, fc = M - 2, 1
    W, S = inputs(E, N, V, M, zero_col=(t - 1, zc), full_col=(t - 1, fc))
    prm = params(variant, liquid, N)
    ev = event_list(E, M, n, t, zc, fc)
    plain = engine.run(variant, prm, W, S, want_hist=hist)
    assert bool((plain.C[t - 1, :, zc] == 0).all()) and bool((plain.C[t - 1, :, fc] != 0).all())  # the plants decide
    got, ref = check(variant, prm, W, S, ev, want_hist=hist, shape=shape)
    # the comparison is not of equal zeros: the resets changed the final state of scenario n, and of no other
    assert not torch.equal(bits(got.B_final[n]), bits(plain.B_final[n]))
    for k in NAMES[:3]:
        assert torch.equal(bits(getattr(got, k)[:, :n]), bits(getattr(plain, k)[:, :n])), k
    assert torch.equal(bits(got.B_final[:n]), bits(plain.B_final[:n]))
    if hist:
        assert torch.equal(bits(got.B_hist[:, :n]), bits(plain.B_hist[:, :n]))
    # the conditional events: zc fired, fc did not (the last epoch's update starts from 0 in column zc alone)
    only_fc = [e for e in ev if e[2] != zc or e[3] != IF_ZERO]
    other = engine.run(variant, prm, W, S, resets=only_fc, want_hist=hist)
    assert not torch.equal(bits(other.B_final[n, :, zc]), bits(got.B_final[n, :, zc]))
    no_fc = [e for e in ev if e[2] != fc or e[3] != IF_ZERO]
    assert_equal(engine.run(variant, prm, W, S, resets=no_fc, want_hist=hist), ref, "without the event that holds")
    # out-of-range events, passed unchecked as a device tensor, change nothing
    dev = torch.tensor(ev + out_of_range(E, N, M, n), dtype=torch.int32, device=engine.device())
    assert_equal(engine.run(variant, prm, W, S, resets=dev, want_hist=hist), ref, "with out-of-range events")
    # with a B_init the events at epoch 0 reach it
    g = torch.Generator().manual_seed(7)
    B0 = torch.rand((N, V, M), generator=g) * (2.0 ** 58 if variant == Y3 else 0.5)
    with_init, _ = check(variant, prm, W, S, ev, B0, want_hist=hist)
    no_e0 = engine.run(variant, prm, W, S, B0, resets=[e for e in ev if e[0] != 0], want_hist=hist)
    if hist:
        assert not torch.equal(bits(with_init.B_hist[0, n, :, 3]), bits(no_e0.B_hist[0, n, :, 3]))
        assert torch.equal(bits(with_init.B_hist[0, n, :, zc]), bits(no_e0.B_hist[0, n, :, zc]))


@pytest.mark.parametrize("variant,liquid", GROUP)
def test_events_in_every_scenario(variant, liquid):
    E, N, V, M = 6, 2, 33, 68
    W, S = inputs(E, N, V, M, zero_col=(3, 66), full_col=(3, 1))
    prm = params(variant, liquid, N)
    ev = event_list(E, M, 0, 4, 66, 1) + [(t, 1, c, ALWAYS) for t, c in ((1, 67), (2, 0), (5, 64))] + [(4, 1, 66, IF_ZERO)]
    check(variant, prm, W, S, ev, want_hist=True)
    check(variant, prm, W, S, ev)


@pytest.mark.parametrize("variant,liquid", GROUP)
@pytest.mark.parametrize("E,N,V,M,hist", [(6, 2, 33, 68, True), (5, 1, 5, 1032, True), (6, 2, 33, 68, False)],
                         ids=["tile_hist", "wide", "no-history"])
def test_strided_and_absent_history(variant, liquid, E, N, V, M, hist):
    W, S = inputs(E, N, V, M, zero_col=(E - 2, M - 2), full_col=(E - 2, 1))
    prm = params(variant, liquid, N)
    ev = event_list(E, M, N - 1, E - 1, M - 2, 1)
    if hist:
        got, _ = check(variant, prm, W, S, ev, want_hist=True, hist_stride=2, hist_first=1)
        assert got.hist_epochs == tuple(range(1, E, 2))
        plan = engine.scan_plan(variant, N, E, V, M, True, hist_stride=2, hist_first=1)
        assert plan.hs and plan.shape in ("tile_hist", "wide")
    else:
        got, _ = check(variant, prm, W, S, ev)
        assert got.B_hist is None


@pytest.mark.parametrize("variant,liquid", GROUP)
@pytest.mark.parametrize("chunk,t", [(2, 2), (3, 3), (2, 4)])
@pytest.mark.parametrize("hist", [False, True], ids=["flat1", "tile_hist"])
def test_conditional_event_at_a_chunks_first_epoch(variant, liquid, chunk, t, hist):
    E, N, V, M = 6, 2, 5, 68
    W, S = inputs(E, N, V, M, zero_col=(t - 1, 7), full_col=(t - 1, 9))
    prm = params(variant, liquid, N)
    ev = [(t, 1, 7, IF_ZERO), (t, 1, 9, IF_ZERO), (t, 0, 64, ALWAYS), (1, 1, 67, ALWAYS)]
    one, ref = check(variant, prm, W, S, ev, want_hist=hist)
    got = engine.run(variant, prm, W, S, resets=ev, want_hist=hist, chunk_epochs=chunk)
    assert got.extra["resets_path"] == "native"
    assert_equal(got, ref, f"chunk_epochs={chunk}")
    fired = engine.run(variant, prm, W, S, resets=[(t, 1, 7, ALWAYS), (t, 0, 64, ALWAYS), (1, 1, 67, ALWAYS)],
                       want_hist=hist, chunk_epochs=chunk)
    assert_equal(fired, ref, "the conditional event fired on the previous chunk's consensus")


@pytest.mark.parametrize("variant,liquid,mode", [pytest.param(Y3, False, ALWAYS, id="yuma31"),
                                                 pytest.param(Y3, False, IF_ZERO, id="yuma32"),
                                                 pytest.param(Y4, True, IF_ZERO, id="yuma4-liquid")])
@pytest.mark.parametrize("hist", [False, True], ids=["flat1", "tile_hist"])
def test_events_beside_the_params_own_reset(variant, liquid, mode, hist):
    E, N, V, M = 6, 2, 5, 68
    W, S = inputs(E, N, V, M, zero_col=(2, 5))
    own = params(variant, liquid, N, reset_mode=mode, reset_epoch=3, reset_index=5, n_miners=M, n_epochs=E)
    plain = params(variant, liquid, N)
    ev = [(2, 1, 66, ALWAYS), (3, 1, 5, ALWAYS), (3, 0, 6, ALWAYS), (4, 1, 0, ALWAYS)]
    folded = ev + [(3, n, 5, mode) for n in range(N)]
    got, ref = check(variant, own, W, S, ev, want_hist=hist, chain_events=folded, chain_prm=plain)
    # the own reset did something: without it scenario 0 ends elsewhere
    without = engine.run(variant, plain, W, S, resets=ev, want_hist=hist)
    assert not torch.equal(bits(without.B_final[0]), bits(got.B_final[0]))


@pytest.mark.parametrize("variant,name", [(Y3, orc.YUMA3), (Y4, orc.YUMA4)], ids=["yuma3", "yuma4"])
def test_oracle_with_the_events_applied_by_hand(variant, name):
    E, N, V, M = 5, 2, 32, 200
    W, S = synth.weights(0x5EED5, E, N, V, M), synth.stakes(0x5EED5, E, N, V, period=2)
    cfgs = [YumaConfig(yuma_params=YumaParams(bond_alpha=0.1 + 0.07 * i, decay_rate=0.1 + 0.03 * i,
                                              capacity_alpha=0.1 + 0.02 * i)) for i in range(N)]
    ev = [(1, 1, 0, ALWAYS), (2, 0, 199, ALWAYS), (2, 1, -1, ALWAYS), (3, 1, 64, IF_ZERO), (4, 0, 3, ALWAYS),
          (4, 1, 3, IF_ZERO), (0, 0, 1, ALWAYS)]
    got = engine.run(variant, [engine.make_params(variant, c) for c in cfgs], torch.from_numpy(W), torch.from_numpy(S),
                     resets=ev, want_hist=True)
    torch.cuda.synchronize()
    assert got.extra["resets_path"] == "native"
    for n in range(N):
        B, Cp = None, None
        for t in range(E):
            for te, ne, c, mode in ev:
                if te == t and ne == n and B is not None:
                    if mode == ALWAYS or (Cp is not None and c >= 0 and Cp[c] == 0.0):
                        B = B.copy()
                        B[:, slice(None) if c < 0 else c] = 0.0
            res = orc.epoch(name, W[t, n], S[t, n], B, cfgs[n])
            B, Cp = res["validator_bonds"], res["server_consensus_weight"]
            np.testing.assert_array_equal(got.C[t, n].cpu().numpy(), Cp)
            np.testing.assert_allclose(got.Dn[t, n].cpu().numpy(), res["validator_reward_normalized"], rtol=1e-5, atol=1e-7)
            np.testing.assert_allclose(got.B_hist[t, n].cpu().numpy(), B, rtol=1e-5, atol=1e-6 * float(np.abs(B).max()))


# ---------------------------------------------------------------------------
# graphs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant,liquid", GROUP)
@pytest.mark.parametrize("E,N,V,M,hist", [(6, 2, 5, 260, False), (6, 2, 33, 68, True)], ids=["flat1", "tile_hist"])
def test_graph_replays_and_rereads_the_list(variant, liquid, E, N, V, M, hist):
    W, S = inputs(E, N, V, M, zero_col=(3, 7), full_col=(3, 9))
    prm = params(variant, liquid, N)
    dev = engine.device()
    first = [(1, 1, 0, ALWAYS), (4, 1, 7, IF_ZERO), (4, 1, 9, IF_ZERO), (2, 0, M - 1, ALWAYS), (E, 0, 0, ALWAYS)]
    second = [(5, 0, 3, ALWAYS), (4, 0, 7, IF_ZERO), (2, 1, -1, ALWAYS), (1, 1, 64, ALWAYS), (1, 1, 64, ALWAYS)]
    lst = torch.tensor(first, dtype=torch.int32, device=dev)
    d0 = engine.run(variant, prm, W, S, resets=first[:-1], want_hist=hist)
    d1 = engine.run(variant, prm, W, S, resets=second, want_hist=hist)
    assert not torch.equal(bits(d0.B_final), bits(d1.B_final))
    g = engine.RunGraph(variant, prm, W, S, resets=lst, want_hist=hist)
    try:
        assert g.result.extra["resets_path"] == "native" and g.result.extra["resets"] is lst
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


def test_an_empty_list_is_the_plain_run():
    W, S = inputs(6, 2, 5, 260)
    prm = params(Y3, False, 2)
    plain = engine.run(Y3, prm, W, S)
    got = engine.run(Y3, prm, W, S, resets=[])
    assert got.extra["resets_path"] == "native"
    for k in NAMES:
        assert torch.equal(bits(getattr(got, k)), bits(getattr(plain, k))), k


# ---------------------------------------------------------------------------
# fallbacks: the chain itself
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant,liquid", GROUP)
@pytest.mark.parametrize("hist", [False, True], ids=["no-history", "history"])
def test_the_scalar_form_takes_the_segments(variant, liquid, hist):
    E, N, V, M = 6, 2, 9, 10  # M % 4 != 0
    W, S = inputs(E, N, V, M, zero_col=(3, 7), full_col=(3, 5))
    own = params(variant, liquid, N, reset_mode=ALWAYS, reset_epoch=2, reset_index=1, n_miners=M, n_epochs=E)
    ev = [(1, 1, 9, ALWAYS), (4, 1, 7, IF_ZERO), (4, 1, 5, IF_ZERO), (5, 0, -1, ALWAYS), (1, 1, 9, ALWAYS)]
    folded = ev + [(2, n, 1, ALWAYS) for n in range(N)]
    assert not engine.resets_native(variant, N, E, V, M, hist)
    kw = dict(hist_stride=2, hist_first=1) if hist else {}
    got, _ = check(variant, own, W, S, ev, path="segments", want_hist=hist, chain_events=folded,
                   chain_prm=params(variant, liquid, N), **kw)
    plain = engine.run(variant, params(variant, liquid, N), W, S)
    assert not torch.equal(bits(got.B_final), bits(plain.B_final))
    # a device list is read back for the chain; what the device code would ignore is ignored here too
    dev = torch.tensor(ev + out_of_range(E, N, M, 1), dtype=torch.int32, device=engine.device())
    again = engine.run(variant, own, W, S, resets=dev, want_hist=hist, **kw)
    assert again.extra["resets_path"] == "segments"
    for k in NAMES:
        assert torch.equal(bits(getattr(again, k)), bits(getattr(got, k))), k
    with pytest.raises(engine.EngineError, match="resets"):
        engine.RunGraph(variant, own, W, S, resets=ev, want_hist=hist)


def test_shared_inputs_take_the_segments():
    E, V, M = 6, 6, 8
    W, S = inputs(E, 1, V, M, zero_col=(3, 7))
    prm = params(Y3, False, 3)
    ev = [(1, 1, 0, ALWAYS), (4, 2, 7, IF_ZERO), (2, 0, -1, ALWAYS), (5, 1, 3, ALWAYS)]
    got, _ = check(Y3, prm, W, S, ev, path="segments", want_hist=True, shared_inputs=True)
    plain = engine.run(Y3, prm, W, S, shared_inputs=True)
    assert not torch.equal(bits(got.B_final), bits(plain.B_final))
    with pytest.raises(engine.EngineError, match="resets"):
        engine.RunGraph(Y3, prm, W, S, resets=ev, shared_inputs=True)


@pytest.mark.parametrize("variant,liquid", GROUP)
def test_uint16_weights_take_the_segments(variant, liquid):
    E, N, V, M = 6, 2, 5, 68
    g = torch.Generator().manual_seed(11)
    W = torch.randint(0, 65536, (E, N, V, M), generator=g, dtype=torch.int32).to(torch.uint16)
    _, S = inputs(E, N, V, M)
    prm = params(variant, liquid, N)
    ev = [(1, 1, 0, ALWAYS), (4, 1, 67, ALWAYS), (2, 0, 64, ALWAYS), (3, 1, -1, ALWAYS)]
    got, _ = check(variant, prm, W, S, ev, path="segments", want_hist=True)
    assert got.extra["w_path"] == "u16"
    with pytest.raises(engine.EngineError, match="resets"):
        engine.RunGraph(variant, prm, W, S, resets=ev)


# ---------------------------------------------------------------------------
# the public surface
# ---------------------------------------------------------------------------
@dataclass
class FourServers(BaseCase):
    """A case of the built-in kind with four servers: M % 4 == 0, the vector form."""
    name: str = "Four servers - the validators move one by one"
    validators: list[str] = field(default_factory=lambda: ["Big vali. (0.8)", "Small vali. (0.1)", "Small vali. 2 (0.1)"])
    base_validator: str = "Big vali. (0.8)"
    num_epochs: int = 12
    servers: list[str] = field(default_factory=lambda: ["Server 1", "Server 2", "Server 3", "Server 4"])
    weight_schedule = (
        (0, 2, ((1.0, 0.0, 0.0, 0.0), (0.5, 0.5, 0.0, 0.0), (0.25, 0.25, 0.25, 0.25))),
        (3, 6, ((0.0, 1.0, 0.0, 0.0), (0.5, 0.5, 0.0, 0.0), (0.0, 0.0, 0.5, 0.5))),
        (7, LAST, ((0.0, 0.0, 0.7, 0.3), (0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 0.5, 0.5))),
    )


VERSIONS = ("Yuma 3.1 (Rhef+reset)", "Yuma 3.2 (Rhef+conditional)", "Yuma 4 (Rhef+relative bonds)", "Yuma 3 (Rhef)")


def test_run_simulations_bond_resets():
    case = FourServers()
    runs = [SimulationRun(case, v, YumaConfig()) for v in VERSIONS]
    pairs = [[(3, 0), (5, 1), (5, 3), (8, 0), (8, 0), (1, 2), (40, 1)], [(3, 2), (4, 0), (9, 1), (8, 0)],
             [(3, 3), (8, 0), (2, 1)], [(3, 0), (5, 1)]]
    ref = run_simulations(runs)
    got = run_simulations(runs, bond_resets=pairs)
    W, S = case.packed_inputs()
    E, V, M = W.shape
    changed = []
    for k, (run, (div, bonds, inc)) in enumerate(zip(runs, got)):
        variant, mode = simulation_utils.resolve_version(run.yuma_version)
        ev = [(e, 0, i, mode) for e, i in pairs[k] if e < E] if mode != engine.RESET_NONE else []
        prm = [engine.make_params(variant, run.yuma_config)]
        c = chain(variant, prm, W[:, None], S[:, None], None, ev, want_hist=True)
        assert len(bonds) == E and len(inc) == E
        assert all(torch.equal(bits(b), bits(c["B_hist"][t, 0].cpu())) for t, b in enumerate(bonds))
        assert all(torch.equal(bits(x), bits(c["I"][t, 0].cpu())) for t, x in enumerate(inc))
        assert div == simulation_utils._dividends_per_1000_tao(case, run.yuma_config, S, c["Dn"][:, 0].cpu())
        changed.append(any(not torch.equal(bits(a), bits(b)) for a, b in zip(bonds, ref[k][1])))
    assert changed[0] and changed[1] and not changed[3]  # 3.1 and 3.2 reset something; plain Yuma 3 ignores the pairs
    assert got[3][0] == ref[3][0]
