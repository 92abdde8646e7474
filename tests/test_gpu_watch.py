"""Watched bond columns (gpu marker): engine.run(..., watch=cols) and
RunGraph(..., watch=cols), run_simulations(..., bonds_columns=).

Every comparison is bit equality of B_watch with B_hist[..., cols] of the run
WITHOUT a watch list; Dn, C, I and B_final must equal that run's too (the main
path's launches are unchanged). Inputs are random weights with planted exact
zeros, a zero-stake validator and an all-zero weight row. The shapes are the
smallest that reach each branch of k_bonds_watch and of its host code: row
guards (V x n_watch no multiple of the 64-thread block), M % 4 != 0 (scalar
main run), several blocks per scenario with per-scenario parameters, every
reset mode on a watched and on an unwatched column, chunks, resumed runs, the
history stride, a schedule, uint16 weights, both histories at once, more than
1024 validators, a replayed graph whose list is rewritten in place, the dense
fallback of the column-normalised variants, the oracle and the public surface."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from conftest import assert_close
from oracle import yuma_oracle as orc

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
# one Yuma 3 and one Yuma 4 liquid parameter set per group
GROUP = [pytest.param(Y3, False, id="yuma3"), pytest.param(Y4, True, id="yuma4-liquid")]
VERSION = {Y3: "Yuma 3 (Rhef)", Y4: "Yuma 4 (Rhef+relative bonds) - liquid alpha on"}


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
                      yuma_params=YumaParams(bond_alpha=0.1 + 0.07 * i, liquid_alpha=liquid,
                                             decay_rate=0.1 + 0.03 * i, capacity_alpha=0.1 + 0.02 * i))


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
        # (the rest of that epoch dense, so that the other columns' consensus sums to more than the
        # half level a zero column's bisection bound would otherwise quantise to at so few miners)
        e = zero_col[0]
        W[e] = 0.5 + 0.5 * torch.rand((N, V, M), generator=g)
        W[e, :, 1 % V, :] = 0.0
        W[e, :, :, zero_col[1]] = 0.0
    if full_col is not None:
        W[full_col[0], :, :, full_col[1]] = 0.5
    return W, S


def check(variant, prm, W, S, cols, B_init=None, *, ref_kw=None, native=True, **kw):
    """run(watch=cols) against the run without a watch list: B_watch ==
    B_hist[..., cols] of the history run, Dn / C / I / B_final those of the
    plain run, bit for bit. Returns (watched run, history run)."""
    ref_kw = kw if ref_kw is None else ref_kw
    hist = engine.run(variant, prm, W, S, B_init, want_hist=True, **ref_kw)
    plain = engine.run(variant, prm, W, S, B_init, **ref_kw)
    got = engine.run(variant, prm, W, S, B_init, watch=cols, **kw)
    torch.cuda.synchronize()
    assert got.extra["watch_path"] == ("native" if native else "dense")
    assert got.B_hist is None and got.watch_cols == tuple(int(c) for c in cols)
    assert got.hist_epochs == hist.hist_epochs
    idx = torch.as_tensor(list(cols), device=hist.B_hist.device, dtype=torch.long)
    want = hist.B_hist.index_select(3, idx)
    assert got.B_watch.dtype == torch.float32 and got.B_watch.shape == want.shape
    assert torch.equal(bits(got.B_watch), bits(want)), "B_watch != B_hist[..., cols]"
    for name in ("Dn", "C", "I", "B_final"):
        assert torch.equal(bits(getattr(got, name)), bits(getattr(plain, name))), name
    assert torch.equal(bits(got.B_final), bits(hist.B_final))
    return got, hist


@pytest.mark.parametrize("variant,liquid", GROUP)
@pytest.mark.parametrize("cols", [[7, 0, 7], [3]], ids=["last-first-duplicate", "one"])
def test_base_case(variant, liquid, cols):
    W, S = inputs(6, 2, 5, 8)
    got, hist = check(variant, params(variant, liquid, 2), W, S, cols)
    assert got.hist_epochs == tuple(range(6))
    assert float(hist.B_hist.abs().max()) > 0  # (the comparison is not of zeros)


@pytest.mark.parametrize("variant,liquid", GROUP)
@pytest.mark.parametrize("V,M,cols", [
    pytest.param(67, 12, [11, 4, 0], id="row-guards"),   # 201 elements: no multiple of a block, M % 8 == 4
    pytest.param(9, 10, [9, 2], id="non-vector-M"),      # M % 4 != 0: the scalar main run
])
def test_odd_shapes(variant, liquid, V, M, cols):
    W, S = inputs(6, 2, V, M)
    check(variant, params(variant, liquid, 2), W, S, cols)


@pytest.mark.parametrize("variant,liquid", GROUP)
def test_several_blocks_per_scenario_with_different_parameters(variant, liquid):
    N, V, M, E = 3, 300, 72, 12  # 1500 elements = 24 blocks per scenario, the last one part-filled
    W, S = inputs(E, N, V, M)
    prm = params(variant, liquid, N)
    if liquid:  # one fixed-alpha scenario among the liquid ones
        prm[1] = engine.make_params(variant, config(False, 1))
    got, hist = check(variant, prm, W, S, [71, 5, 64, 0, 33])
    assert not torch.equal(bits(got.B_watch[:, 0]), bits(got.B_watch[:, 1]))


RESET_E, RESET_T = 8, 3


@pytest.mark.parametrize("on_watched", [True, False], ids=["watched", "unwatched"])
@pytest.mark.parametrize("variant,liquid,mode,fires", [
    pytest.param(Y3, False, engine.RESET_ALWAYS, True, id="yuma31"),
    pytest.param(Y3, False, engine.RESET_IF_ZERO_CONSENSUS, True, id="yuma32-fires"),
    pytest.param(Y3, False, engine.RESET_IF_ZERO_CONSENSUS, False, id="yuma32-holds"),
    pytest.param(Y4, True, engine.RESET_IF_ZERO_CONSENSUS, True, id="yuma4-fires"),
    pytest.param(Y4, True, engine.RESET_IF_ZERO_CONSENSUS, False, id="yuma4-holds"),
])
def test_resets(variant, liquid, mode, fires, on_watched):
    V, M, cols = 5, 8, [6, 2]
    col = 6 if on_watched else 4
    conditional = mode == engine.RESET_IF_ZERO_CONSENSUS
    # a zero consensus at the epoch before the reset makes the conditional reset fire
    W, S = inputs(RESET_E, 2, V, M, zero_col=(RESET_T - 1, col) if conditional and fires else None,
                  full_col=(RESET_T - 1, col) if conditional and not fires else None)
    prm = params(variant, liquid, 2, reset_mode=mode, reset_epoch=RESET_T, reset_index=col, n_miners=M,
                 n_epochs=RESET_E)
    got, hist = check(variant, prm, W, S, cols)
    if conditional:  # the plant decides the branch
        zero = bool((hist.C[RESET_T - 1, :, col] == 0).all())
        assert zero == fires
    if on_watched:
        # the state after the reset epoch restarts from zero exactly when the reset fired
        norst = engine.run(variant, params(variant, liquid, 2), W, S, want_hist=True)
        same = torch.equal(bits(norst.B_hist[RESET_T:, :, :, col]), bits(hist.B_hist[RESET_T:, :, :, col]))
        assert same != fires


def test_reset_all_columns():
    V, M = 5, 8
    W, S = inputs(RESET_E, 2, V, M)
    prm = params(Y3, False, 2, reset_mode=engine.RESET_ALWAYS, reset_epoch=RESET_T, reset_index=None, n_miners=M,
                 n_epochs=RESET_E)
    assert prm[0].flags & engine.FLAG_RESET_ALL_COLUMNS
    check(Y3, prm, W, S, [6, 2])


@pytest.mark.parametrize("variant,liquid", GROUP)
def test_chunks_equal_one_chunk(variant, liquid):
    W, S = inputs(10, 2, 5, 8, zero_col=(5, 7))  # (the conditional reset fires on the previous chunk's consensus)
    prm = params(variant, liquid, 2, reset_mode=engine.RESET_IF_ZERO_CONSENSUS if variant == Y4 else engine.RESET_ALWAYS,
                 reset_epoch=6, reset_index=7, n_miners=8, n_epochs=10)  # the reset epoch starts a chunk
    check(variant, prm, W, S, [7, 0, 7], chunk_epochs=3, ref_kw={})


@pytest.mark.parametrize("variant,liquid", GROUP)
def test_resumed_run_equals_the_second_half(variant, liquid):
    E, H, cols = 10, 5, [7, 0, 7]
    W, S = inputs(E, 2, 5, 8)
    prm = params(variant, liquid, 2)
    whole = engine.run(variant, prm, W, S, want_hist=True)
    first = engine.run(variant, prm, W[:H], S[:H])
    idx = torch.as_tensor(cols, device=whole.B_hist.device)
    # dense: every epoch of the second half
    second = engine.run(variant, prm, W[H:], S[H:], first.B_final, watch=cols)
    assert second.extra["watch_path"] == "native"
    assert torch.equal(bits(second.B_watch), bits(whole.B_hist[H:].index_select(3, idx)))
    assert torch.equal(bits(second.B_final), bits(whole.B_final))
    # stride 3 from epoch 1 of the whole run stores 1, 4, 7: hist_first keeps the phase (7 - 5 = 2)
    assert engine.hist_epochs(E, 3, 1) == (1, 4, 7)
    second = engine.run(variant, prm, W[H:], S[H:], first.B_final, watch=cols, hist_stride=3, hist_first=2)
    assert second.hist_epochs == (2,)
    assert torch.equal(bits(second.B_watch), bits(whole.B_hist[7:8].index_select(3, idx)))


@pytest.mark.parametrize("variant,liquid", GROUP)
@pytest.mark.parametrize("stride,first,epochs", [
    (3, 1, (1, 4, 7)),
    (10, None, (9,)),     # a stride of E: the last epoch alone
    (15, 2, (2,)),        # a stride above E
    (15, None, ()),       # ... whose first stored epoch lies past the run: no slot
])
def test_stride(variant, liquid, stride, first, epochs):
    W, S = inputs(10, 2, 5, 8)
    got, _ = check(variant, params(variant, liquid, 2), W, S, [7, 0, 7], hist_stride=stride, hist_first=first,
                   chunk_epochs=4)
    assert got.hist_epochs == epochs and got.B_watch.shape[0] == len(epochs)


@pytest.mark.parametrize("variant,liquid", GROUP)
def test_schedule(variant, liquid):
    K, sched = 3, [0, 1, 1, 2, 0, 0, 2, 1, 2]
    W, S = inputs(K, 2, 5, 8)
    got, hist = check(variant, params(variant, liquid, 2), W, S, [7, 0, 7], sched=sched, chunk_epochs=4)
    assert got.extra["sched_path"] == "native" and hist.extra["sched_path"] == "native"
    assert got.hist_epochs == tuple(range(9))
    # ... and equals the run on the expanded inputs
    exp = engine.run(variant, params(variant, liquid, 2), W[sched], S[sched], want_hist=True)
    assert torch.equal(bits(got.B_watch), bits(exp.B_hist[..., [7, 0, 7]]))


@pytest.mark.parametrize("variant,liquid", GROUP)
def test_uint16_weights(variant, liquid):
    E, N, V, M = 6, 2, 8, 8
    g = torch.Generator().manual_seed(16)
    Wf = torch.randint(0, 65536, (E, N, V, M), generator=g)
    Wf[torch.rand((E, N, V, M), generator=g) < 0.2] = 0
    Wf[:, :, 1, :] = 0
    W = Wf.to(torch.uint16)
    S = torch.rand((E, N, V), generator=g) + 0.25
    S[:, :, V - 1] = 0.0
    got, hist = check(variant, params(variant, liquid, 2), W, S, [7, 0, 7])
    assert got.extra["w_path"] == "u16" and hist.extra["w_path"] == "u16"
    # the widened run holds the same bits
    wide = engine.run(variant, params(variant, liquid, 2), Wf.to(torch.float32), S, want_hist=True)
    assert torch.equal(bits(got.B_watch), bits(wide.B_hist[..., [7, 0, 7]]))


@pytest.mark.parametrize("variant,liquid", GROUP)
def test_both_histories_in_one_run(variant, liquid):
    W, S = inputs(6, 2, 5, 8)
    cols = [7, 0, 7]
    for kw in ({}, {"hist_stride": 2}, {"hist_dtype": torch.bfloat16}):
        r = engine.run(variant, params(variant, liquid, 2), W, S, want_hist=True, watch=cols, **kw)
        assert r.extra["watch_path"] == "native" and r.B_hist is not None
        assert r.B_watch.shape[0] == r.B_hist.shape[0] == len(r.hist_epochs)
        if "hist_dtype" in kw:  # YUMA_RUN_HIST_BF16 concerns B_hist only: B_watch stays fp32
            assert r.B_hist.dtype == torch.bfloat16 and r.extra["hist_path"] == "bf16"
            assert torch.equal(bits(r.B_watch.to(torch.bfloat16)), bits(r.B_hist[..., cols]))
        else:
            assert torch.equal(bits(r.B_watch), bits(r.B_hist[..., cols]))


@pytest.mark.parametrize("variant,liquid", GROUP)
def test_wide_validator_set(variant, liquid):
    W, S = inputs(3, 1, 1030, 8)  # above 1024 validators: the streamed phase 1
    check(variant, params(variant, liquid, 1), W, S, [7, 0, 7])


@pytest.mark.parametrize("variant,liquid", GROUP)
def test_graph_replays_and_follows_the_list_in_place(variant, liquid):
    W, S = inputs(6, 2, 5, 8)
    prm = params(variant, liquid, 2)
    hist = engine.run(variant, prm, W, S, want_hist=True).B_hist
    dev = hist.device
    lst = torch.tensor([7, 0, 7], dtype=torch.int32, device=dev)
    direct = engine.run(variant, prm, W, S, watch=lst)
    assert direct.extra["watch"] is lst
    g = engine.RunGraph(variant, prm, W, S, watch=lst)
    try:
        assert g.result.extra["watch"] is lst and g.result.extra["watch_path"] == "native"
        for _ in range(2):
            g.result.B_watch.fill_(float("nan"))
            r = g.launch()
            torch.cuda.synchronize()
            assert torch.equal(bits(r.B_watch), bits(direct.B_watch))
            assert torch.equal(bits(r.B_watch), bits(hist[..., [7, 0, 7]]))
            assert torch.equal(bits(r.Dn), bits(direct.Dn)) and torch.equal(bits(r.B_final), bits(direct.B_final))
        lst.copy_(torch.tensor([1, 6, 2], dtype=torch.int32))
        r = g.launch()
        torch.cuda.synchronize()
        assert torch.equal(bits(r.B_watch), bits(hist[..., [1, 6, 2]]))
    finally:
        g.close()


@pytest.mark.parametrize("variant", [Y1, RUST], ids=["yuma1", "yuma0"])
def test_fallback_gathers_a_dense_history(variant):
    W, S = inputs(6, 2, 6, 8)
    prm = [engine.make_params(variant, config(variant == Y1, i)) for i in range(2)]
    assert not engine.watch_native(variant, 2, 6, 6, 8, 3)
    check(variant, prm, W, S, [7, 0, 7], native=False)
    check(variant, prm, W, S, [7, 0, 7], native=False, hist_stride=2)
    both = engine.run(variant, prm, W, S, want_hist=True, watch=[7, 0, 7])
    assert both.extra["watch_path"] == "dense" and both.B_hist is not None
    assert torch.equal(bits(both.B_watch), bits(both.B_hist[..., [7, 0, 7]]))
    with pytest.raises(engine.EngineError, match="watch"):
        engine.RunGraph(variant, prm, W, S, watch=[7, 0, 7])


def test_shared_inputs_fall_back_too():
    W, S = inputs(6, 1, 6, 8)
    prm = params(Y3, False, 3)
    got = engine.run(Y3, prm, W, S, shared_inputs=True, watch=[7, 0])
    hist = engine.run(Y3, prm, W, S, shared_inputs=True, want_hist=True)
    assert got.extra["watch_path"] == "dense" and got.B_hist is None
    assert torch.equal(bits(got.B_watch), bits(hist.B_hist[..., [7, 0]]))


@pytest.mark.parametrize("variant,liquid", GROUP)
def test_oracle_at_the_watched_columns(variant, liquid):
    E, V, M, cols = 8, 5, 8, [7, 0, 3]
    W, S = inputs(E, 1, V, M)
    S[:, :, V - 1] = 0.125  # (the oracle comparison keeps every validator staked)
    cfg = config(liquid, 0)
    got = engine.run(variant, [engine.make_params(variant, cfg)], W, S, watch=cols)
    ref = orc.run(VERSION[variant], W[:, 0].numpy(), S[:, 0].numpy(), cfg)
    assert_close(got.B_watch[:, 0].cpu().numpy(), ref["B"][:, :, cols], what="B at the watched columns")


@pytest.mark.parametrize("kw", [{}, {"bonds_every": 2}, {"dedup_inputs": True},
                                {"bonds_every": 2, "dedup_inputs": True}],
                         ids=["default", "every2", "dedup", "every2-dedup"])
def test_run_simulations_bonds_columns(kw):
    versions = ("Yuma 3 (Rhef)", "Yuma 4 (Rhef+relative bonds) - liquid alpha on", "Yuma 1 (paper)")
    runs = [SimulationRun(case, v, YumaConfig(yuma_params=YumaParams(liquid_alpha="liquid" in v)))
            for case in builtin_cases[:2] for v in versions]
    ref = run_simulations(runs, **kw)
    got = run_simulations(runs, bonds_columns=[1, 0], **kw)
    for (d0, b0, i0), (d1, b1, i1) in zip(ref, got):
        assert d0 == d1 and len(b0) == len(b1) > 0
        for x, y in zip(b0, b1):
            assert y.shape == (x.shape[0], 2)
            assert torch.equal(bits(y), bits(x[:, [1, 0]]))
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(i0, i1))
    # a bfloat16 request converts the small fp32 watched history
    g16 = run_simulations(runs[:1], bonds_columns=[1, 0], bonds_dtype=torch.bfloat16, **kw)
    assert all(y.dtype == torch.bfloat16 and torch.equal(bits(y), bits(x[:, [1, 0]].to(torch.bfloat16)))
               for x, y in zip(ref[0][1], g16[0][1]))
