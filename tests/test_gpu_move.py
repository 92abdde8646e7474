"""Bond movement per epoch (gpu marker): engine.run(..., want_move=True),
RunGraph(..., want_move=True) and run_simulations(..., bonds_movement=True).

The reference is the definition: the run with want_hist=True and, on its dense
fp32 history with B_init (or zeros) prepended, (hist[t] - hist[t-1]).abs()
.amax((-2, -1)) and hist[t].abs().amax((-2, -1)) by torch. Every comparison is
bit equality (NaN entries: equal NaN masks); Dn, C, I and B_final must equal the
plain run's. Inputs are random weights with planted exact zeros, a zero-stake
validator and an all-zero weight row. The shapes are the smallest that cross
each boundary of the reduction: one block, several row and column blocks of
the one-row flat scan (4 rows x 256 miners per block), the two-row flat scan
(from 4096 blocks), more than 1024 validators; a planted maximum at each corner
of the block grid and in another scenario; resets, resumes, chunks, uint16
weights, schedules, a watch list, a history in the same run, NaN, replayed
graphs, the dense fallbacks and the public surface."""

from __future__ import annotations

from dataclasses import dataclass, field

import pytest
import torch

pytestmark = pytest.mark.gpu

from yuma_simulation._internal import engine  # noqa: E402
from yuma_simulation._internal import simulation_utils  # noqa: E402
from yuma_simulation._internal.cases import LAST, BaseCase  # noqa: E402
from yuma_simulation._internal.cases import cases as builtin_cases  # noqa: E402
from yuma_simulation._internal.simulation_utils import SimulationRun, run_simulations  # noqa: E402
from yuma_simulation._internal.yumas import (  # noqa: E402
    SimulationHyperparameters,
    YumaConfig,
    YumaParams,
)

RUST, Y1, Y2, Y3, Y4 = (engine.VARIANT_RUST, engine.VARIANT_YUMA1, engine.VARIANT_YUMA2,
                        engine.VARIANT_YUMA3, engine.VARIANT_YUMA4)
# Yuma 3, Yuma 4 and Yuma 4 liquid
GROUP3 = [pytest.param(Y3, False, id="yuma3"), pytest.param(Y4, False, id="yuma4"),
          pytest.param(Y4, True, id="yuma4-liquid")]
GROUP = [GROUP3[0], GROUP3[2]]


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
    """W [E,N,V,M], S [E,N,V]: random weights, a fifth of them exact zeros,
    validator 1's weights all zero, the last validator without stake.
    zero_col = (epoch, column): that column of that epoch all zero, so that its
    consensus is exactly 0; full_col = (epoch, column): every validator weights
    it, so that its consensus is not 0."""
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


def reference(hist, B_init):
    """B_move of a dense fp32 history [E, N, V, M], by the definition."""
    first = torch.zeros_like(hist[:1]) if B_init is None else B_init.to(hist.device, torch.float32)[None]
    full = torch.cat([first, hist])
    return torch.stack([(full[1:] - full[:-1]).abs().amax((-2, -1)), hist.abs().amax((-2, -1))], dim=-1)


def assert_move_equal(got, want, what="B_move"):
    assert got.dtype == torch.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    nan_g, nan_w = torch.isnan(got), torch.isnan(want)
    assert torch.equal(nan_g, nan_w), f"{what}: NaN masks differ"
    g, w = bits(torch.where(nan_g, torch.zeros_like(got), got)), bits(torch.where(nan_w, torch.zeros_like(want), want))
    if not torch.equal(g, w):
        bad = (g != w).nonzero()[:5].tolist()
        raise AssertionError(f"{what} differs at {bad}: {[float(got[tuple(i)]) for i in bad]} != "
                             f"{[float(want[tuple(i)]) for i in bad]}")


def check(variant, prm, W, S, B_init=None, *, path="native", ref_kw=None, plain_kw=None, shape=None, **kw):
    """run(want_move=True) against the definition on the history run of the same
    call, and against the plain run (the same run without want_move: plain_kw
    where it asks for more than ref_kw) for every other output. Returns (the
    movement run, the history run)."""
    ref_kw = kw if ref_kw is None else ref_kw
    hist = engine.run(variant, prm, W, S, B_init, want_hist=True, **ref_kw)
    plain = engine.run(variant, prm, W, S, B_init, **(ref_kw if plain_kw is None else plain_kw))
    got = engine.run(variant, prm, W, S, B_init, want_move=True, **kw)
    torch.cuda.synchronize()
    assert got.extra["move_path"] == path
    E, N = hist.B_hist.shape[:2]
    assert got.B_move.shape == (E, N, 2) and got.B_move.is_cuda
    assert_move_equal(got.B_move, reference(hist.B_hist, B_init))
    for name in ("Dn", "C", "I", "B_final"):
        assert torch.equal(bits(getattr(got, name)), bits(getattr(plain, name))), name
    if path == "native":
        assert got.B_hist is None
    if shape is not None:  # the scan the movement run reaches
        V, M = W.shape[2:]
        plan = engine.scan_plan(variant, N, E, V, M, w_u16=got.extra["w_path"] == "u16",
                                sched=got.extra.get("sched_path") == "native")
        assert plan.form == "k_bonds_elem" and plan.shape == shape[0] and (plan.rowblocks, plan.cblocks) == shape[1:], plan
    return got, hist


# ---------------------------------------------------------------------------
# the shapes: every boundary of the reduction
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant,liquid", GROUP3)
@pytest.mark.parametrize("E,N,V,M,shape", [
    pytest.param(6, 2, 4, 8, ("flat1", 1, 1), id="flat1-one-block"),
    pytest.param(6, 2, 5, 260, ("flat1", 2, 2), id="flat1-2x2-blocks"),   # rows >= V and quads >= M in the last blocks
    pytest.param(4, 64, 512, 8, ("flat2", 64, 1), id="flat2"),            # 64 * 64 * 1 = 4096 two-row blocks
    pytest.param(3, 1, 1030, 8, ("flat1", 258, 1), id="above-1024-validators"),
])
def test_shapes(variant, liquid, E, N, V, M, shape):
    W, S = inputs(E, N, V, M)
    got, hist = check(variant, params(variant, liquid, N), W, S, shape=shape)
    assert not bool((got.B_move == 0).any())  # (the comparison is not of zeros: every epoch moves)
    if N > 1:
        assert not torch.equal(bits(got.B_move[:, 0]), bits(got.B_move[:, 1]))


def test_flat2_threshold_is_where_the_test_puts_it():
    assert engine.scan_plan(Y3, 64, 4, 512, 8).shape == "flat2"
    assert engine.scan_plan(Y3, 63, 4, 512, 8).shape == "flat1"


# ---------------------------------------------------------------------------
# the maximum's position: one large element of B_init in a small state. The
# first epoch's movement (and size) is that element's, whichever block holds it.
# ---------------------------------------------------------------------------
PV, PM = 5, 260   # 2 x 2 blocks of 4 rows x 256 miners per scenario


@pytest.mark.parametrize("variant,liquid", GROUP)
@pytest.mark.parametrize("n,v,m", [
    pytest.param(0, 0, 0, id="first"),
    pytest.param(0, PV - 1, PM - 1, id="last"),
    pytest.param(0, 3, 256, id="last-row-of-block-0-first-column-of-block-1"),
    pytest.param(2, 2, 130, id="scenario-2"),
])
def test_the_planted_maximum_is_found(variant, liquid, n, v, m):
    E, N = 3, 3
    W, S = inputs(E, N, PV, PM)
    S[:, :, PV - 1] = 0.125  # (every row staked: the Yuma 3 cap of the planted row is not zero)
    big, small = (2.0 ** 62, 2.0 ** 40) if variant == Y3 else (0.75, 1e-3)
    B_init = torch.full((N, PV, PM), small)
    B_init[n, v, m] = big
    got, hist = check(variant, params(variant, liquid, N), W, S, B_init, shape=("flat1", 2, 2))
    h0 = hist.B_hist[0].cpu()
    # the planted element is the first epoch's largest movement and largest bond of its scenario alone
    d0 = (h0 - B_init).abs()
    assert int(d0[n].argmax()) == v * PM + m
    assert float(got.B_move[0, n, 0]) == float(d0[n, v, m])
    for other in range(N):  # (no leak: the other scenarios' entries stay those of their own small states)
        if other != n:
            assert float(got.B_move[0, other, 0]) < float(got.B_move[0, n, 0])
            assert float(got.B_move[0, other, 1]) < float(got.B_move[0, n, 1])


# ---------------------------------------------------------------------------
# resets and resumes
# ---------------------------------------------------------------------------
RESET_E, RESET_T = 8, 3


@pytest.mark.parametrize("variant,liquid,mode,fires", [
    pytest.param(Y3, False, engine.RESET_ALWAYS, True, id="yuma31"),
    pytest.param(Y3, False, engine.RESET_IF_ZERO_CONSENSUS, True, id="yuma32-fires"),
    pytest.param(Y3, False, engine.RESET_IF_ZERO_CONSENSUS, False, id="yuma32-holds"),
    pytest.param(Y4, True, engine.RESET_IF_ZERO_CONSENSUS, True, id="yuma4-fires"),
    pytest.param(Y4, True, engine.RESET_IF_ZERO_CONSENSUS, False, id="yuma4-holds"),
])
def test_resets(variant, liquid, mode, fires):
    V, M, col = 5, 8, 6
    conditional = mode == engine.RESET_IF_ZERO_CONSENSUS
    W, S = inputs(RESET_E, 2, V, M, zero_col=(RESET_T - 1, col) if conditional and fires else None,
                  full_col=(RESET_T - 1, col) if conditional and not fires else None)
    prm = params(variant, liquid, 2, reset_mode=mode, reset_epoch=RESET_T, reset_index=col, n_miners=M,
                 n_epochs=RESET_E)
    got, hist = check(variant, prm, W, S)
    if conditional:  # the plant decides the branch
        assert bool((hist.C[RESET_T - 1, :, col] == 0).all()) == fires
    # before the reset epoch, and throughout when it does not fire, the run without a reset moves alike
    norst = engine.run(variant, params(variant, liquid, 2), W, S, want_move=True)
    assert torch.equal(bits(norst.B_move[:RESET_T]), bits(got.B_move[:RESET_T]))
    if not fires:
        assert torch.equal(bits(norst.B_move), bits(got.B_move))


def test_reset_all_columns():
    V, M = 5, 8
    W, S = inputs(RESET_E, 2, V, M)
    prm = params(Y3, False, 2, reset_mode=engine.RESET_ALWAYS, reset_epoch=RESET_T, reset_index=None, n_miners=M,
                 n_epochs=RESET_E)
    assert prm[0].flags & engine.FLAG_RESET_ALL_COLUMNS
    check(Y3, prm, W, S)


@pytest.mark.parametrize("variant,liquid", GROUP)
def test_b_init_given_and_resumed_run(variant, liquid):
    E, H = 10, 5
    W, S = inputs(E, 2, 5, 8)
    prm = params(variant, liquid, 2)
    whole, _ = check(variant, prm, W, S)                      # B_init NULL: B_{-1} is zeros
    first = engine.run(variant, prm, W[:H], S[:H])
    second, _ = check(variant, prm, W[H:], S[H:], first.B_final.clone())   # B_init given
    assert torch.equal(bits(second.B_move), bits(whole.B_move[H:]))
    assert torch.equal(bits(second.B_final), bits(whole.B_final))


@pytest.mark.parametrize("variant,liquid", GROUP)
def test_chunks_equal_one_chunk(variant, liquid):
    E = 10
    W, S = inputs(E, 2, 5, 8, zero_col=(5, 7))  # (the conditional reset fires on the previous chunk's consensus)
    prm = params(variant, liquid, 2, reset_mode=engine.RESET_IF_ZERO_CONSENSUS if variant == Y4 else engine.RESET_ALWAYS,
                 reset_epoch=6, reset_index=7, n_miners=8, n_epochs=E)  # the reset epoch starts a chunk
    one = None
    for chunk in (1, 3, E):
        got, _ = check(variant, prm, W, S, chunk_epochs=chunk, ref_kw={})
        one = got if one is None else one
        assert torch.equal(bits(got.B_move), bits(one.B_move)), chunk


def test_more_epochs_than_the_parking_buffer_holds():
    """The wave's maxima are parked for up to 256 epochs before they are sent."""
    E = 300
    W, S = inputs(4, 1, 5, 8)
    sched = [(7 * t) % 4 for t in range(E)]
    check(Y3, params(Y3, False, 1), W, S, sched=sched)
    check(Y4, params(Y4, True, 1), W[sched], S[sched])


# ---------------------------------------------------------------------------
# combinations
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant,liquid", GROUP)
def test_uint16_weights(variant, liquid):
    E, N, V, M = 6, 2, 8, 8
    g = torch.Generator().manual_seed(16)
    Wf = torch.randint(0, 65536, (E, N, V, M), generator=g)
    Wf[torch.rand((E, N, V, M), generator=g) < 0.2] = 0
    Wf[:, :, 1, :] = 0
    S = torch.rand((E, N, V), generator=g) + 0.25
    S[:, :, V - 1] = 0.0
    got, hist = check(variant, params(variant, liquid, 2), Wf.to(torch.uint16), S, shape=("flat1", 2, 1))
    assert got.extra["w_path"] == "u16" and hist.extra["w_path"] == "u16"
    wide = engine.run(variant, params(variant, liquid, 2), Wf.to(torch.float32), S, want_move=True)
    assert wide.extra["w_path"] == "f32" and torch.equal(bits(got.B_move), bits(wide.B_move))


@pytest.mark.parametrize("variant,liquid", GROUP)
@pytest.mark.parametrize("K,sched", [(3, [0, 1, 1, 2, 0, 0, 2, 1, 2]), (1, [0] * 7)], ids=["K3", "K1"])
def test_schedule(variant, liquid, K, sched):
    W, S = inputs(K, 2, 5, 8)
    got, hist = check(variant, params(variant, liquid, 2), W, S, sched=sched, chunk_epochs=4, shape=("flat1", 2, 1))
    assert got.extra["sched_path"] == "native" and hist.extra["sched_path"] == "native"
    exp = engine.run(variant, params(variant, liquid, 2), W[sched], S[sched], want_move=True)
    assert torch.equal(bits(got.B_move), bits(exp.B_move))


@pytest.mark.parametrize("variant,liquid", GROUP)
def test_schedule_with_uint16_weights(variant, liquid):
    g = torch.Generator().manual_seed(17)
    W = torch.randint(0, 65536, (3, 2, 8, 8), generator=g).to(torch.uint16)
    S = torch.rand((3, 2, 8), generator=g) + 0.25
    got, _ = check(variant, params(variant, liquid, 2), W, S, sched=[0, 2, 1, 1, 0])
    assert got.extra["w_path"] == "u16" and got.extra["sched_path"] == "native"


@pytest.mark.parametrize("variant,liquid", GROUP)
def test_watch_list_in_the_same_run(variant, liquid):
    cols = [7, 0, 7]
    W, S = inputs(6, 2, 5, 8)
    got, hist = check(variant, params(variant, liquid, 2), W, S, watch=cols, ref_kw={})
    assert got.extra["watch_path"] == "native"
    assert torch.equal(bits(got.B_watch), bits(hist.B_hist[..., cols]))
    got, _ = check(variant, params(variant, liquid, 2), W, S, watch=cols, hist_stride=2, ref_kw={})
    assert got.hist_epochs == (1, 3, 5) and torch.equal(bits(got.B_watch), bits(hist.B_hist[1::2][..., cols]))


@pytest.mark.parametrize("variant,liquid", GROUP)
@pytest.mark.parametrize("kw", [{}, {"hist_stride": 2}, {"hist_dtype": torch.bfloat16},
                                {"hist_stride": 3, "hist_first": 1, "hist_dtype": torch.bfloat16}],
                         ids=["dense", "stride2", "bf16", "stride3-bf16"])
def test_history_in_the_same_run_takes_the_dense_path(variant, liquid, kw):
    W, S = inputs(7, 2, 5, 8)
    prm = params(variant, liquid, 2)
    alone = engine.run(variant, prm, W, S, want_hist=True, **kw)
    got, _ = check(variant, prm, W, S, path="dense", want_hist=True, ref_kw={}, plain_kw=dict(want_hist=True, **kw),
                   **kw)
    assert got.hist_epochs == alone.hist_epochs and got.B_hist.dtype == alone.B_hist.dtype
    assert torch.equal(bits(got.B_hist), bits(alone.B_hist))
    with pytest.raises(engine.EngineError, match="want_move"):
        engine.RunGraph(variant, prm, W, S, want_hist=True, want_move=True, **kw)


# ---------------------------------------------------------------------------
# NaN
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant,liquid", GROUP)
def test_nan_stays_in_its_scenario(variant, liquid):
    W, S = inputs(5, 2, 5, 260)
    B_init = torch.full((2, 5, 260), 0.25)
    clean = engine.run(variant, params(variant, liquid, 2), W, S, B_init.clone(), want_move=True)
    B_init[1, 4, 257] = float("nan")
    got, hist = check(variant, params(variant, liquid, 2), W, S, B_init)
    assert bool(torch.isnan(got.B_move[0, 1]).all())             # the first epoch's difference and size
    assert not bool(torch.isnan(got.B_move[:, 0]).any())
    assert torch.equal(bits(got.B_move[:, 0]), bits(clean.B_move[:, 0]))


# ---------------------------------------------------------------------------
# graphs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant,liquid", GROUP)
def test_graph_replays_start_from_zero(variant, liquid):
    W, S = inputs(6, 2, 5, 260)
    prm = params(variant, liquid, 2)
    dev = engine.device()
    B0 = torch.full((2, 5, 260), 0.5 if variant == Y4 else 2.0 ** 60, device=dev)
    B1 = torch.zeros((2, 5, 260), device=dev)
    d0 = engine.run(variant, prm, W, S, B0.clone(), want_move=True)
    d1 = engine.run(variant, prm, W, S, B1.clone(), want_move=True)
    assert float(d0.B_move[0, 0, 0]) > float(d1.B_move[0, 0, 0])  # (a missing re-zero would keep d0's maxima)
    buf = B0.clone()
    g = engine.RunGraph(variant, prm, W, S, buf, want_move=True)
    try:
        assert g.result.extra["move_path"] == "native"
        for want in (d0, d0, d1):
            if want is d1:
                buf.copy_(B1)  # refilled in place between two replays
            r = g.launch()
            torch.cuda.synchronize()
            assert_move_equal(r.B_move, want.B_move)
            assert torch.equal(bits(r.B_final), bits(want.B_final))
    finally:
        g.close()


# ---------------------------------------------------------------------------
# fallbacks: a dense history, reduced on the device
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [Y1, RUST], ids=["yuma1", "yuma0"])
def test_other_variants_fall_back(variant):
    W, S = inputs(6, 2, 6, 8)
    prm = [engine.make_params(variant, config(variant == Y1, i)) for i in range(2)]
    assert not engine.move_native(variant, 2, 6, 6, 8)
    got, _ = check(variant, prm, W, S, path="dense")
    assert got.B_hist is None  # dropped again: nobody asked for it
    with pytest.raises(engine.EngineError, match="want_move"):
        engine.RunGraph(variant, prm, W, S, want_move=True)


def test_shared_inputs_and_the_scalar_form_fall_back():
    W, S = inputs(6, 1, 6, 8)
    prm = params(Y3, False, 3)
    got, _ = check(Y3, prm, W, S, path="dense", shared_inputs=True)
    assert got.B_hist is None
    with pytest.raises(engine.EngineError, match="want_move"):
        engine.RunGraph(Y3, prm, W, S, shared_inputs=True, want_move=True)
    W, S = inputs(6, 2, 9, 10)  # M % 4 != 0
    got, _ = check(Y4, params(Y4, True, 2), W, S, path="dense")
    assert got.B_hist is None
    with pytest.raises(engine.EngineError, match="want_move"):
        engine.RunGraph(Y4, params(Y4, True, 2), W, S, want_move=True)


@pytest.mark.parametrize("variant,liquid", GROUP)
@pytest.mark.parametrize("sched", [None, [0, 1, 1, 2, 0, 0, 2, 1, 2]], ids=["per-epoch", "schedule"])
def test_a_buffer_off_its_alignment_falls_back(variant, liquid, sched):
    """Native by its sizes, but B_init is a view 4 bytes off a 16-byte boundary:
    the scalar form, so the dense path -- on the inputs and the schedule as given."""
    N, V, M = 2, 5, 8
    W, S = inputs(3 if sched else 9, N, V, M)
    prm = params(variant, liquid, N)
    kw = {} if sched is None else {"sched": sched}
    assert engine.move_native(variant, N, 9, V, M)
    g = torch.Generator().manual_seed(5)
    b0 = torch.rand((N, V, M), generator=g) * (2.0 ** 58 if variant == Y3 else 0.5)
    buf = torch.empty(N * V * M + 1, device=engine.device())
    B_init = buf[1:].view(N, V, M)
    B_init.copy_(b0)
    assert B_init.data_ptr() % 16 == 4
    got, hist = check(variant, prm, W, S, B_init, path="dense", **kw)
    assert got.B_hist is None and got.B_move.shape == (9, N, 2)
    if sched is not None:
        assert hist.extra["sched_path"] == "expanded"
        plain = engine.run(variant, prm, W[sched], S[sched], B_init, want_hist=True)
        assert_move_equal(got.B_move, reference(plain.B_hist, B_init))
    # the aligned call is native and gives the same movement
    aligned = engine.run(variant, prm, W, S, b0, want_move=True, **kw)
    assert aligned.extra["move_path"] == "native"
    assert_move_equal(got.B_move, aligned.B_move)
    with pytest.raises(engine.EngineError, match="captured run"):
        engine.RunGraph(variant, prm, W, S, B_init, want_move=True, **kw)


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


VERSIONS = ("Yuma 3 (Rhef)", "Yuma 4 (Rhef+relative bonds) - liquid alpha on", "Yuma 1 (paper)")


def sim_runs():
    return [SimulationRun(case, v, YumaConfig(yuma_params=YumaParams(liquid_alpha="liquid" in v)))
            for case in (builtin_cases[0], builtin_cases[1], FourServers()) for v in VERSIONS]


def test_run_simulations_bonds_movement():
    runs = sim_runs()
    ref = run_simulations(runs)
    assert all(len(t) == 3 for t in ref)
    got = run_simulations(runs, bonds_movement=True)
    for (d0, b0, i0), t in zip(ref, got):
        assert len(t) == 4
        d1, b1, i1, mv = t
        assert d0 == d1 and len(b0) == len(b1) > 0
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(b0, b1))
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(i0, i1))
        E = len(b0)
        assert mv.shape == (E, 2) and mv.dtype == torch.float32 and not mv.is_cuda
        hist = torch.stack(b0)[:, None]  # [E, 1, V, M]
        assert_move_equal(mv, reference(hist, None)[:, 0])
        assert not bool((mv[:, 0] == 0).all())  # (the comparison is not of zeros)
        assert 0 <= int(engine.settled_epoch(mv, 1e-3, relative=True)) <= E
    # with columns and a bfloat16 history the first three elements are the call's without the keyword
    a = run_simulations(runs, bonds_columns=[1, 0], bonds_dtype=torch.bfloat16, bonds_every=2)
    b = run_simulations(runs, bonds_columns=[1, 0], bonds_dtype=torch.bfloat16, bonds_every=2, bonds_movement=True)
    for x, y, r in zip(a, b, ref):
        assert len(x) == 3 and len(y) == 4
        assert x[0] == y[0] and all(torch.equal(bits(p), bits(q)) for p, q in zip(x[1], y[1])) and len(x[1]) == len(y[1])
        assert_move_equal(y[3], reference(torch.stack(r[1])[:, None], None)[:, 0])


@pytest.mark.parametrize("kw", [{}, {"bonds_every": 2, "dedup_inputs": True}], ids=["default", "every2-dedup"])
def test_run_simulations_without_bonds_keeps_no_history(monkeypatch, kw):
    """want_bonds=False with bonds_movement=True, the intended use: a Yuma 3 /
    Yuma 4 group in vector form (the four-server case) makes one engine call,
    native, and no engine call of it asks for or returns a [V, M] history."""
    runs = sim_runs()
    ref = run_simulations(runs)
    seen = []
    real = engine.run

    def spy(*a, **k):
        r = real(*a, **k)
        seen.append((a[0], int(a[2].shape[-1]), k, r))
        return r

    monkeypatch.setattr(simulation_utils.engine, "run", spy)
    lean = run_simulations(runs, want_bonds=False, bonds_movement=True, **kw)
    outer = [(v, M, k, r) for v, M, k, r in seen if k.get("want_move")]
    assert sorted((v, M) for v, M, k, r in outer) == sorted((v, M) for v in (Y1, Y3, Y4) for M in (2, 4))
    for v, M, k, r in outer:
        E, N, _ = r.B_move.shape
        native = v in (Y3, Y4) and M == 4
        assert native == engine.move_native(v, N, E, 3, M)
        assert r.extra["move_path"] == ("native" if native else "dense")
        assert r.B_hist is None and r.hist_epochs is None and not k.get("want_hist")
    # a native group makes no second engine call: only the fallbacks run an inner history run
    inner = [(v, M) for v, M, k, r in seen if not k.get("want_move")]
    assert sorted(inner) == sorted((v, M) for v, M, k, r in outer if not (v in (Y3, Y4) and M == 4))
    assert all(r.B_hist is None for v, M, k, r in seen if v in (Y3, Y4) and M == 4)
    for (d0, b0, i0), t in zip(ref, lean):
        assert len(t) == 4 and t[1] == [] and t[0] == d0
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(i0, t[2]))
        assert_move_equal(t[3], reference(torch.stack(b0)[:, None], None)[:, 0])
