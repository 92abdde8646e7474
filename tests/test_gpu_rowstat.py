"""Per-validator bond summary per epoch (gpu marker): engine.run(...,
want_row_stats=True), RunGraph(..., want_row_stats=True) and
run_simulations(..., bonds_row_stats=True).

The reference is always the dense fp32 history of a plain engine.run(...,
want_hist=True), reduced by torch, with B_init (or zeros) prepended. Columns 0
and 1 of B_rowstat are compared bit for bit with (hist[t] - hist[t-1]).abs()
.amax(-1) and hist[t].abs().amax(-1) (NaN entries: equal NaN masks), and their
amax over v with the B_move of a want_move run. Column 2, the row total, is
compared with the float64 row sum of the history under the bound
    |x - ref| <= (M - 1) * 2^-24 * ref,
which is derived, not measured: every term is a non-negative finite fp32 (the
test asserts so on the history), and for such terms a sum of M terms in any
order is within gamma_(M-1) of the exact sum. (A row of the history that holds
a NaN -- a planted one, or a liquid-alpha scenario of the recipe whose
bond_alpha turned NaN -- must have a NaN total instead.) Between runs of the native path
column 2 is compared bit for bit: across chunk_epochs, across the two flat scan
shapes, with and without watch lists. Dn, C, I and B_final must equal the plain
run's. The inputs follow tests/test_gpu_move.py: random weights with planted
exact zeros, a zero-stake validator and an all-zero weight row. The history run
of a case is made once and shared by the tests that need it."""

from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu

from yuma_simulation._internal import engine  # noqa: E402
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
# (E, N, V, M) -> the scan shape and its (row blocks, column blocks)
SHAPES = {
    (6, 2, 5, 260): ("flat1", 2, 2),      # 2 x 2 blocks, part-filled row and column blocks
    (4, 64, 512, 8): ("flat2", 64, 1),    # two rows per lane
    (3, 1, 1030, 8): ("flat1", 258, 1),   # above 1024 validators
    (19, 2, 9, 520): ("flat1", 3, 3),     # more epochs than one 16-epoch DP_QTE run, three column blocks
}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "gpu tests need a ROCm GPU"
    engine.load_library()
    yield
    _HIST.clear()
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


def inputs(E, N, V, M, seed=0):
    """W [E,N,V,M], S [E,N,V]: random weights, a fifth of them exact zeros,
    validator 1's weights all zero, the last validator without stake."""
    g = torch.Generator().manual_seed(1000 * V + M + seed)
    W = torch.rand((E, N, V, M), generator=g)
    W[torch.rand((E, N, V, M), generator=g) < 0.2] = 0.0
    W[:, :, 1 % V, :] = 0.0
    S = torch.rand((E, N, V), generator=g) + 0.25
    S[:, :, V - 1] = 0.0
    return W, S


_HIST: dict = {}


def history(key, variant, prm, W, S, B_init=None, **kw):
    """The plain history run of a case, made once (key names the case)."""
    if key not in _HIST:
        _HIST[key] = engine.run(variant, prm, W, S, B_init, want_hist=True, **kw)
        torch.cuda.synchronize()
    return _HIST[key]


def reference(hist, B_init):
    """Columns 0 and 1 of B_rowstat of a dense fp32 history [E, N, V, M], by the definition."""
    first = torch.zeros_like(hist[:1]) if B_init is None else B_init.to(hist.device, torch.float32)[None]
    full = torch.cat([first, hist])
    return torch.stack([(full[1:] - full[:-1]).abs().amax(-1), hist.abs().amax(-1)], dim=-1)


def assert_bits_equal(got, want, what):
    assert got.dtype == torch.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    nan_g, nan_w = torch.isnan(got), torch.isnan(want)
    assert torch.equal(nan_g, nan_w), f"{what}: NaN masks differ"
    g, w = bits(torch.where(nan_g, torch.zeros_like(got), got)), bits(torch.where(nan_w, torch.zeros_like(want), want))
    if not torch.equal(g, w):
        bad = (g != w).nonzero()[:5].tolist()
        raise AssertionError(f"{what} differs at {bad}: {[float(got[tuple(i)]) for i in bad]} != "
                             f"{[float(want[tuple(i)]) for i in bad]}")


def assert_totals_within_bound(total, hist):
    """|x - ref| <= (M - 1) 2^-24 ref against the float64 row sum; the bound
    holds for non-negative finite terms, which is asserted first. The recipe's
    liquid-alpha scenarios can end in a NaN bond_alpha, and with it an all-NaN
    bond state, in the existing history run; a row that holds a NaN has no
    bound: its float64 sum is a NaN, and so must its total be. Every other row
    must be non-negative and finite and is held to the bound."""
    h = hist.cpu()
    nan_row = torch.isnan(h).any(-1)
    h = torch.where(nan_row[..., None], torch.zeros_like(h), h)
    assert bool(torch.isfinite(h).all()) and bool((h >= 0).all()), "the bound needs a non-negative finite history"
    assert not bool(nan_row.all()), "every row holds a NaN: nothing is compared"
    M = h.shape[-1]
    ref = h.double().sum(-1)
    x = total.cpu().double()
    assert torch.equal(torch.isnan(x), nan_row), "a total is NaN exactly where its row holds a NaN"
    x = torch.where(nan_row, torch.zeros_like(x), x)
    err, bound = (x - ref).abs(), (M - 1) * 2.0 ** -24 * ref
    print(f"row totals: max |x - ref| / ref = {float((err / ref.clamp_min(1e-300)).max()):.3e}, "
          f"bound {(M - 1) * 2.0 ** -24:.3e}")
    assert bool((err <= bound).all()), (float((err - bound).max()), (err > bound).nonzero()[:5].tolist())


def check(variant, prm, W, S, B_init=None, *, hist, path="native", shape=None, **kw):
    """run(want_row_stats=True) against the definition on the history run of the
    same call and, for every other output, against that run too (a history run
    keeps the plain run's Dn, C, I and B_final: tests/test_gpu_parity.py)."""
    got = engine.run(variant, prm, W, S, B_init, want_row_stats=True, **kw)
    torch.cuda.synchronize()
    assert got.extra["rowstat_path"] == path
    E, N, V, M = hist.B_hist.shape
    assert got.B_rowstat.shape == (E, N, V, 3) and got.B_rowstat.is_cuda and got.B_rowstat.dtype == torch.float32
    assert_bits_equal(got.B_rowstat[..., :2].contiguous(), reference(hist.B_hist, B_init), "B_rowstat[..., :2]")
    assert_totals_within_bound(got.B_rowstat[..., 2], hist.B_hist)
    for name in ("Dn", "C", "I", "B_final"):  # (a NaN's payload is not part of the comparison across scan shapes)
        assert_bits_equal(getattr(got, name), getattr(hist, name), name)
    if path == "native" and not kw.get("want_hist"):
        assert got.B_hist is None
    if shape is not None:
        plan = engine.scan_plan(variant, N, E, V, M)
        assert plan.form == "k_bonds_elem" and plan.shape == shape[0] and (plan.rowblocks, plan.cblocks) == shape[1:], plan
    return got


# ---------------------------------------------------------------------------
# the shapes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant,liquid", GROUP3)
@pytest.mark.parametrize("E,N,V,M", list(SHAPES), ids=["flat1-2x2", "flat2", "above-1024-validators", "19-epochs-3-cblocks"])
def test_shapes(variant, liquid, E, N, V, M):
    W, S = inputs(E, N, V, M)
    prm = params(variant, liquid, N)
    hist = history(("shape", variant, liquid, E, N, V, M), variant, prm, W, S)
    got = check(variant, prm, W, S, hist=hist, shape=SHAPES[(E, N, V, M)])
    # amax over v of columns 0 and 1 is B_move of a want_move run, bit for bit
    mv = engine.run(variant, prm, W, S, want_move=True)
    assert mv.extra["move_path"] == "native"
    assert_bits_equal(got.B_rowstat[..., :2].amax(2), mv.B_move, "amax over v")
    # the plain run's outputs
    plain = engine.run(variant, prm, W, S)
    for name in ("Dn", "C", "I", "B_final"):
        assert torch.equal(bits(getattr(got, name)), bits(getattr(plain, name))), name
    assert not bool((got.B_rowstat[..., 0].amax(2) == 0).any())  # (the comparison is not of zeros: every epoch moves)
    assert bool((got.B_rowstat[..., 2] > 0).any())
    if N > 1:
        assert not torch.equal(bits(got.B_rowstat[:, 0]), bits(got.B_rowstat[:, 1]))


def test_flat2_threshold_is_where_the_test_puts_it():
    assert engine.scan_plan(Y3, 64, 4, 512, 8).shape == "flat2"
    assert engine.scan_plan(Y3, 63, 4, 512, 8).shape == "flat1"


@pytest.mark.parametrize("variant,liquid", GROUP3)
def test_totals_have_the_same_bits_on_both_flat_shapes(variant, liquid):
    """One input, 64 scenarios on the two-row shape and its first 63 on the one-row shape."""
    E, N, V, M = 4, 64, 512, 8
    W, S = inputs(E, N, V, M)
    prm = params(variant, liquid, N)
    two = engine.run(variant, prm, W, S, want_row_stats=True)
    one = engine.run(variant, prm[:63], W[:, :63].contiguous(), S[:, :63].contiguous(), want_row_stats=True)
    assert two.extra["rowstat_path"] == one.extra["rowstat_path"] == "native"
    assert_bits_equal(one.B_rowstat, two.B_rowstat[:, :63].contiguous(), "flat1 against flat2")


@pytest.mark.parametrize("variant,liquid", GROUP3)
def test_totals_do_not_depend_on_the_chunking(variant, liquid):
    E, N, V, M = 19, 2, 9, 520
    W, S = inputs(E, N, V, M)
    prm = params(variant, liquid, N)
    hist = history(("shape", variant, liquid, E, N, V, M), variant, prm, W, S)
    one = None
    for chunk in (0, 1, 5):
        got = check(variant, prm, W, S, hist=hist, chunk_epochs=chunk)
        one = got if one is None else one
        assert_bits_equal(got.B_rowstat, one.B_rowstat, f"chunk_epochs={chunk}")


@pytest.mark.parametrize("variant,liquid", GROUP)
def test_watch_lists_in_the_same_run(variant, liquid):
    E, N, V, M = 6, 2, 5, 260
    cols, rows = [259, 0, 7], [4, 0]
    W, S = inputs(E, N, V, M)
    prm = params(variant, liquid, N)
    hist = history(("shape", variant, liquid, E, N, V, M), variant, prm, W, S)
    alone = check(variant, prm, W, S, hist=hist)
    for kw in (dict(watch=cols), dict(watch_rows=rows), dict(watch=cols, watch_rows=rows)):
        got = check(variant, prm, W, S, hist=hist, **kw)
        assert_bits_equal(got.B_rowstat, alone.B_rowstat, str(kw))
        if "watch" in kw:
            assert got.extra["watch_path"] == "native"
            assert torch.equal(bits(got.B_watch), bits(hist.B_hist[..., cols]))
        if "watch_rows" in kw:
            assert got.extra["rows_path"] == "native"
            assert torch.equal(bits(got.B_rows), bits(hist.B_hist[:, :, rows]))


# ---------------------------------------------------------------------------
# B_init, the parameter record's reset, NaN
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant,liquid", GROUP)
def test_b_init_given(variant, liquid):
    """Epoch 0's movement is against B_init; a resumed run continues the whole run's summary."""
    E, H, N, V, M = 10, 5, 2, 5, 8
    W, S = inputs(E, N, V, M)
    prm = params(variant, liquid, N)
    whole = check(variant, prm, W, S, hist=history(("whole", variant, liquid), variant, prm, W, S))
    first = engine.run(variant, prm, W[:H], S[:H])
    B0 = first.B_final.clone()
    second = check(variant, prm, W[H:], S[H:], B0, hist=history(("second", variant, liquid), variant, prm, W[H:], S[H:], B0))
    assert_bits_equal(second.B_rowstat, whole.B_rowstat[H:].contiguous(), "the resumed half")
    zeros = engine.run(variant, prm, W[H:], S[H:], want_row_stats=True)
    assert not torch.equal(bits(zeros.B_rowstat[0, ..., 0]), bits(second.B_rowstat[0, ..., 0]))


@pytest.mark.parametrize("variant,liquid", GROUP)
def test_the_params_reset_shows_as_movement_at_its_epoch(variant, liquid):
    E, T, N, V, M, col = 8, 3, 2, 5, 8, 6
    W, S = inputs(E, N, V, M)
    prm = params(variant, liquid, N, reset_mode=engine.RESET_ALWAYS, reset_epoch=T, reset_index=col, n_miners=M, n_epochs=E)
    hist = history(("reset", variant, liquid), variant, prm, W, S)
    got = check(variant, prm, W, S, hist=hist)
    norst = engine.run(variant, params(variant, liquid, N), W, S, want_row_stats=True)
    assert torch.equal(bits(norst.B_rowstat[:T]), bits(got.B_rowstat[:T]))
    # at the reset epoch the reset column's own step is in its rows' movement: B[v][col] went from its old value to
    # the update of 0
    h = hist.B_hist
    step = (h[T, :, :, col] - h[T - 1, :, :, col]).abs()
    assert bool((got.B_rowstat[T, :, :, 0] >= step).all()) and bool((step > 0).any())
    assert not torch.equal(bits(norst.B_rowstat[T]), bits(got.B_rowstat[T]))


@pytest.mark.parametrize("variant,liquid", GROUP)
def test_nan_stays_in_its_row(variant, liquid):
    E, N, V, M = 5, 2, 5, 260
    W, S = inputs(E, N, V, M)
    prm = params(variant, liquid, N)
    B_init = torch.full((N, V, M), 0.25)
    clean = engine.run(variant, prm, W, S, B_init.clone(), want_row_stats=True)
    B_init[1, 3, 257] = float("nan")
    hist = history(("nan", variant, liquid), variant, prm, W, S, B_init)
    got = check(variant, prm, W, S, B_init, hist=hist)
    assert bool(torch.isnan(got.B_rowstat[0, 1, 3, :2]).all())          # the first epoch's difference and size
    nan_rows = torch.isnan(got.B_rowstat[..., :2]).any(-1)
    assert not bool(nan_rows[0, 0].any()) and not bool(nan_rows[0, 1, [0, 1, 2, 4]].any())
    # every other row keeps the clean run's summary
    assert_bits_equal(got.B_rowstat[:, 0].contiguous(), clean.B_rowstat[:, 0].contiguous(), "scenario 0")
    assert_bits_equal(got.B_rowstat[:, 1, [0, 1, 2, 4]].contiguous(), clean.B_rowstat[:, 1, [0, 1, 2, 4]].contiguous(),
                      "the other rows of scenario 1")


# ---------------------------------------------------------------------------
# graphs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant,liquid", GROUP)
def test_graph_replays_start_from_zero(variant, liquid):
    """Two replays with W rewritten in place in between, each bit-equal to the direct run of its weights. The first
    replay's weights sit on a third fewer miners, so its rows' largest bonds are larger: maxima left over from it
    would show in the second replay."""
    E, N, V, M = 6, 2, 5, 260
    W1, S = inputs(E, N, V, M)
    W0 = W1.clone()
    W0[:, :, :, ::3] = 0.0
    prm = params(variant, liquid, N)
    dev = engine.device()
    d0 = engine.run(variant, prm, W0, S, want_row_stats=True)
    d1 = engine.run(variant, prm, W1, S, want_row_stats=True)
    assert bool((d0.B_rowstat[..., 1] > d1.B_rowstat[..., 1]).any())  # (a missing re-zero would keep d0's maxima)
    buf = W0.to(dev).contiguous()
    g = engine.RunGraph(variant, prm, buf, S, want_row_stats=True)
    try:
        assert g.result.extra["rowstat_path"] == "native"
        for W, want in ((W0, d0), (W1, d1)):
            buf.copy_(W)  # refilled in place between the replays
            r = g.launch()
            torch.cuda.synchronize()
            assert_bits_equal(r.B_rowstat, want.B_rowstat, "replay")
            assert torch.equal(bits(r.B_final), bits(want.B_final))
    finally:
        g.close()


# ---------------------------------------------------------------------------
# fallbacks: a dense history, reduced on the device
# ---------------------------------------------------------------------------
def test_yuma1_falls_back():
    W, S = inputs(6, 2, 6, 8)
    prm = [engine.make_params(Y1, config(True, i)) for i in range(2)]
    assert not engine.rowstat_native(Y1, 2, 6, 6, 8)
    got = check(Y1, prm, W, S, hist=history(("y1",), Y1, prm, W, S), path="dense")
    assert got.B_hist is None  # dropped again: nobody asked for it
    with pytest.raises(engine.EngineError, match="want_row_stats"):
        engine.RunGraph(Y1, prm, W, S, want_row_stats=True)


def test_shared_inputs_and_the_scalar_form_fall_back():
    W, S = inputs(6, 1, 6, 8)
    prm = params(Y3, False, 3)
    got = check(Y3, prm, W, S, hist=history(("shared",), Y3, prm, W, S, shared_inputs=True), path="dense",
                shared_inputs=True)
    assert got.B_hist is None
    with pytest.raises(engine.EngineError, match="want_row_stats"):
        engine.RunGraph(Y3, prm, W, S, shared_inputs=True, want_row_stats=True)
    W, S = inputs(6, 2, 9, 262)  # M % 4 != 0
    prm = params(Y4, True, 2)
    got = check(Y4, prm, W, S, hist=history(("scalar",), Y4, prm, W, S), path="dense")
    assert got.B_hist is None
    with pytest.raises(engine.EngineError, match="want_row_stats"):
        engine.RunGraph(Y4, prm, W, S, want_row_stats=True)


@pytest.mark.parametrize("variant,liquid", GROUP)
def test_history_schedule_or_movement_in_the_same_run_take_the_dense_path(variant, liquid):
    E, N, V, M = 6, 2, 5, 260
    W, S = inputs(E, N, V, M)
    prm = params(variant, liquid, N)
    hist = history(("shape", variant, liquid, E, N, V, M), variant, prm, W, S)
    got = check(variant, prm, W, S, hist=hist, path="dense", want_hist=True)
    assert torch.equal(bits(got.B_hist), bits(hist.B_hist))
    got = check(variant, prm, W, S, hist=hist, path="dense", want_move=True)
    assert_bits_equal(got.B_rowstat[..., :2].amax(2), got.B_move, "amax over v")
    got = check(variant, prm, W, S, hist=hist, path="dense", sched=list(range(E)))
    for kw in (dict(want_hist=True), dict(want_move=True), dict(sched=list(range(E)))):
        with pytest.raises(engine.EngineError, match="want_row_stats"):
            engine.RunGraph(variant, prm, W, S, want_row_stats=True, **kw)


# ---------------------------------------------------------------------------
# the public surface
# ---------------------------------------------------------------------------
def test_run_simulations_bonds_row_stats():
    versions = ("Yuma 3 (Rhef)", "Yuma 4 (Rhef+relative bonds) - liquid alpha on", "Yuma 1 (paper)")
    runs = [SimulationRun(case, v, YumaConfig(yuma_params=YumaParams(liquid_alpha="liquid" in v)))
            for case in (builtin_cases[0], builtin_cases[1]) for v in versions]
    ref = run_simulations(runs)
    got = run_simulations(runs, bonds_row_stats=True)
    both = run_simulations(runs, bonds_row_stats=True, bonds_movement=True)
    for (d0, b0, i0), t, u in zip(ref, got, both):
        assert len(t) == 4 and len(u) == 5
        d1, b1, i1, rs = t
        assert d0 == d1 and len(b0) == len(b1) > 0
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(b0, b1))
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(i0, i1))
        hist = torch.stack(b0)[:, None]  # [E, 1, V, M]
        E, _, V, M = hist.shape
        assert rs.shape == (E, V, 3) and rs.dtype == torch.float32 and not rs.is_cuda
        assert_bits_equal(rs[..., :2].contiguous(), reference(hist, None)[:, 0], "bonds_row_stats")
        assert_totals_within_bound(rs[..., 2], hist[:, 0])
        assert not bool((rs[..., 0] == 0).all())
        assert engine.settled_epoch_rows(rs, 1e-3, relative=True).shape == (V,)
        assert torch.equal(bits(u[4]), bits(rs)) and torch.equal(bits(u[3]), bits(rs[..., :2].amax(1)))
