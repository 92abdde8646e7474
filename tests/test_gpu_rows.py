"""Watched validator rows (gpu marker): engine.run(..., watch_rows=rows) and
RunGraph(..., watch_rows=rows), run_simulations(..., bonds_validators=).

Every comparison is bit equality of B_rows with B_hist[:, :, rows, :] of the
run WITHOUT a row list; Dn, C, I and B_final must equal that run's too (the
main path's launches are unchanged). Inputs are test_gpu_watch's: random
weights, a fifth of them exact zeros, validator 1's row all zero, the last
validator without stake. The shapes are the smallest that reach each branch of
k_bonds_rows and of its host code: both column forms (M % 4 != 0, a buffer off
its alignment), two blocks per row with a part-filled second one in either
form, runs shorter than the input ring and no multiple of it, every reset mode
on each component of a quad and on both quads, chunks, resumed runs, the
history stride, a schedule, uint16 weights, the other outputs beside it, more
than 1024 validators, a replayed graph whose list is rewritten in place, the
dense fallbacks, the oracle and the public surface."""

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
ROWS = [4, 0, 4]  # at V = 5: the zero-stake row, a duplicate


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


def gather(hist, rows):
    idx = torch.as_tensor(list(rows), device=hist.device, dtype=torch.long)
    return hist.index_select(2, idx)


def check(variant, prm, W, S, rows, B_init=None, *, ref_kw=None, native=True, **kw):
    """run(watch_rows=rows) against the run without a row list: B_rows ==
    B_hist[:, :, rows, :] of the history run, Dn / C / I / B_final those of the
    plain run, bit for bit. Returns (watched run, history run)."""
    ref_kw = kw if ref_kw is None else ref_kw
    hist = engine.run(variant, prm, W, S, B_init, want_hist=True, **ref_kw)
    plain = engine.run(variant, prm, W, S, B_init, **ref_kw)
    got = engine.run(variant, prm, W, S, B_init, watch_rows=rows, **kw)
    torch.cuda.synchronize()
    assert got.extra["rows_path"] == ("native" if native else "dense")
    assert got.B_hist is None and got.B_watch is None and got.watch_rows == tuple(int(r) for r in rows)
    assert got.hist_epochs == hist.hist_epochs
    want = gather(hist.B_hist, rows)
    assert got.B_rows.dtype == torch.float32 and got.B_rows.shape == want.shape
    assert torch.equal(bits(got.B_rows), bits(want)), "B_rows != B_hist[:, :, rows, :]"
    for name in ("Dn", "C", "I", "B_final"):
        assert torch.equal(bits(getattr(got, name)), bits(getattr(plain, name))), name
    return got, hist


@pytest.mark.parametrize("variant,liquid", GROUP)
@pytest.mark.parametrize("rows", [ROWS, [1]], ids=["unstaked-first-duplicate", "all-zero-row"])
def test_base_case(variant, liquid, rows):
    W, S = inputs(6, 2, 5, 8)
    got, hist = check(variant, params(variant, liquid, 2), W, S, rows)
    assert got.hist_epochs == tuple(range(6))
    assert float(hist.B_hist.abs().max()) > 0  # (the comparison is not of zeros)
    if rows == ROWS:  # per-scenario parameters (validator 1's bonds are zero in every scenario)
        assert not torch.equal(bits(got.B_rows[:, 0]), bits(got.B_rows[:, 1]))
    else:
        assert float(got.B_rows.abs().max()) == 0


@pytest.mark.parametrize("variant,liquid", GROUP)
@pytest.mark.parametrize("M", [
    pytest.param(6, id="scalar-M6"),      # M % 4 != 0: one column per thread, the scalar main run
    pytest.param(70, id="scalar-M70"),    # two blocks per row, 6 threads in the second
    pytest.param(260, id="vector-M260"),  # 65 quads: two blocks per row, one thread in the second
])
def test_column_forms_and_part_filled_blocks(variant, liquid, M):
    W, S = inputs(6, 2, 5, M)
    got, hist = check(variant, params(variant, liquid, 2), W, S, ROWS)
    assert float(got.B_rows[0, :, 1, M - 1].abs().max()) > 0  # validator 0, epoch 0: the part-filled block's last column is written


@pytest.mark.parametrize("variant,liquid", GROUP)
def test_misaligned_state_takes_one_column_per_thread(variant, liquid):
    """B_init at a 4-byte offset from a 16-byte boundary: the quads' 16-byte
    accesses are out, at an M that would otherwise take them. (The engine does
    not report the chosen form: the bits are the check.)"""
    N, V, M = 2, 5, 8
    W, S = inputs(6, N, V, M)
    dev = engine.device()
    g = torch.Generator().manual_seed(3)
    buf = torch.zeros(N * V * M + 1, dtype=torch.float32, device=dev)
    buf[1:] = (0.3 * torch.rand(N * V * M, generator=g)).to(dev)
    B_init = buf[1:].view(N, V, M)
    assert B_init.data_ptr() % 16 == 4 and B_init.is_contiguous()
    check(variant, params(variant, liquid, N), W, S, ROWS, B_init)


@pytest.mark.parametrize("variant,liquid", GROUP)
@pytest.mark.parametrize("E", [1, 3, 11])
def test_ring_edges(variant, liquid, E):
    """Shorter than the ring of 8 epochs, and no multiple of it."""
    W, S = inputs(E, 2, 5, 8)
    check(variant, params(variant, liquid, 2), W, S, ROWS)


RESET_E, RESET_T = 8, 3


@pytest.mark.parametrize("col", [0, 5, 7])  # first of quad 0, second of quad 1, last of quad 1
@pytest.mark.parametrize("variant,liquid,mode,fires", [
    pytest.param(Y3, False, engine.RESET_ALWAYS, True, id="yuma31"),
    pytest.param(Y3, False, engine.RESET_IF_ZERO_CONSENSUS, True, id="yuma32-fires"),
    pytest.param(Y3, False, engine.RESET_IF_ZERO_CONSENSUS, False, id="yuma32-holds"),
    pytest.param(Y4, True, engine.RESET_IF_ZERO_CONSENSUS, True, id="yuma4-fires"),
    pytest.param(Y4, True, engine.RESET_IF_ZERO_CONSENSUS, False, id="yuma4-holds"),
])
def test_resets(variant, liquid, mode, fires, col):
    V, M = 5, 8
    conditional = mode == engine.RESET_IF_ZERO_CONSENSUS
    W, S = inputs(RESET_E, 2, V, M, zero_col=(RESET_T - 1, col) if conditional and fires else None,
                  full_col=(RESET_T - 1, col) if conditional and not fires else None)
    prm = params(variant, liquid, 2, reset_mode=mode, reset_epoch=RESET_T, reset_index=col, n_miners=M,
                 n_epochs=RESET_E)
    got, hist = check(variant, prm, W, S, ROWS)
    if conditional:  # the plant decides the branch
        assert bool((hist.C[RESET_T - 1, :, col] == 0).all()) == fires
    # the column restarts from zero exactly when the reset fired, and only that column
    norst = engine.run(variant, params(variant, liquid, 2), W, S, watch_rows=ROWS)
    same = torch.equal(bits(norst.B_rows[RESET_T:, :, :, col]), bits(got.B_rows[RESET_T:, :, :, col]))
    assert same != fires
    others = [c for c in range(M) if c != col]
    assert torch.equal(bits(norst.B_rows[..., others]), bits(got.B_rows[..., others]))


def test_reset_all_columns():
    V, M = 5, 8
    W, S = inputs(RESET_E, 2, V, M)
    prm = params(Y3, False, 2, reset_mode=engine.RESET_ALWAYS, reset_epoch=RESET_T, reset_index=None, n_miners=M,
                 n_epochs=RESET_E)
    assert prm[0].flags & engine.FLAG_RESET_ALL_COLUMNS
    check(Y3, prm, W, S, ROWS)


@pytest.mark.parametrize("with_state", [True, False], ids=["B_init", "no-state"])
def test_reset_at_epoch_zero(with_state):
    """reset_epoch = 0: the unconditional reset zeroes a caller's state before
    epoch 0 and is nothing without one (the reset needs an old state)."""
    N, V, M = 2, 5, 8
    W, S = inputs(6, N, V, M)
    prm = params(Y3, False, N, reset_mode=engine.RESET_ALWAYS, reset_epoch=0, reset_index=5, n_miners=M, n_epochs=6,
                 resumed=True)
    assert prm[0].reset_mode == engine.RESET_ALWAYS and prm[0].reset_epoch == 0
    # (Yuma 3's bonds carry the 2^64 scale of the stake cap: a state of order 1 would be rounded away at once)
    B_init = 2.0**60 * torch.rand((N, V, M), generator=torch.Generator().manual_seed(5)) if with_state else None
    got, _ = check(Y3, prm, W, S, ROWS, B_init)
    norst = engine.run(Y3, params(Y3, False, N), W, S, B_init, watch_rows=ROWS)
    assert torch.equal(bits(norst.B_rows[..., 5]), bits(got.B_rows[..., 5])) != with_state


@pytest.mark.parametrize("chunk", [1, 4])
@pytest.mark.parametrize("variant,liquid", GROUP)
def test_chunks_equal_one_chunk(variant, liquid, chunk):
    W, S = inputs(10, 2, 5, 8, zero_col=(3, 7))  # (the conditional reset fires on the previous chunk's consensus)
    prm = params(variant, liquid, 2, reset_mode=engine.RESET_IF_ZERO_CONSENSUS if variant == Y4 else engine.RESET_ALWAYS,
                 reset_epoch=4, reset_index=7, n_miners=8, n_epochs=10)  # the reset epoch starts a chunk
    check(variant, prm, W, S, ROWS, chunk_epochs=chunk, ref_kw={})


@pytest.mark.parametrize("variant,liquid", GROUP)
def test_resumed_run_concatenates_to_the_uncut_run(variant, liquid):
    E, H = 10, 4
    W, S = inputs(E, 2, 5, 8)
    prm = params(variant, liquid, 2)
    assert engine.hist_epochs(E, 3, 1) == (1, 4, 7)
    whole = engine.run(variant, prm, W, S, want_hist=True, hist_stride=3, hist_first=1)
    first = engine.run(variant, prm, W[:H], S[:H], watch_rows=ROWS, hist_stride=3, hist_first=1)
    # hist_first keeps the phase: epoch 4 of the whole run is epoch 0 of the second part
    second = engine.run(variant, prm, W[H:], S[H:], first.B_final, watch_rows=ROWS, hist_stride=3, hist_first=0)
    assert first.hist_epochs == (1,) and second.hist_epochs == (0, 3)
    assert second.extra["rows_path"] == "native"
    both = torch.cat([first.B_rows, second.B_rows])
    assert torch.equal(bits(both), bits(gather(whole.B_hist, ROWS)))
    assert torch.equal(bits(second.B_final), bits(whole.B_final))


@pytest.mark.parametrize("variant,liquid", GROUP)
def test_stride(variant, liquid):
    W, S = inputs(10, 2, 5, 8)
    got, hist = check(variant, params(variant, liquid, 2), W, S, ROWS, hist_stride=3, hist_first=1, chunk_epochs=4)
    assert got.hist_epochs == (1, 4, 7) and got.B_rows.shape[0] == 3
    dense = engine.run(variant, params(variant, liquid, 2), W, S, want_hist=True)
    assert torch.equal(bits(got.B_rows), bits(gather(dense.B_hist[[1, 4, 7]], ROWS)))  # slot s holds epoch 1 + 3 s


@pytest.mark.parametrize("M,path", [(8, "native"), (6, "expanded")])
@pytest.mark.parametrize("variant,liquid", GROUP)
def test_schedule(variant, liquid, M, path):
    K, sched = 3, [0, 2, 2, 0, 2, 0, 0, 2, 0]  # slice 1 is never referenced
    W, S = inputs(K, 2, 5, M)
    got, hist = check(variant, params(variant, liquid, 2), W, S, ROWS, sched=sched, chunk_epochs=4)
    assert got.extra["sched_path"] == path and got.hist_epochs == tuple(range(9))
    # ... and equals the run on the expanded inputs
    exp = engine.run(variant, params(variant, liquid, 2), W[sched], S[sched], want_hist=True)
    assert torch.equal(bits(got.B_rows), bits(gather(exp.B_hist, ROWS)))


@pytest.mark.parametrize("M,path", [(8, "u16"), (6, "f32")])
@pytest.mark.parametrize("variant,liquid", GROUP)
def test_uint16_weights(variant, liquid, M, path):
    """test_gpu_watch's uint16 inputs (8 validators). At 5 validators these
    integer weights drive the liquid fit to NaN, and a NaN's sign bit is not
    defined between the engine's own scans (the history-less and the history
    run of one input disagree on it in B_final), so bit equality needs inputs
    that stay finite."""
    E, N, V = 6, 2, 8
    g = torch.Generator().manual_seed(16)
    Wf = torch.randint(0, 65536, (E, N, V, M), generator=g)
    Wf[torch.rand((E, N, V, M), generator=g) < 0.2] = 0
    Wf[:, :, 1, :] = 0
    W = Wf.to(torch.uint16)
    S = torch.rand((E, N, V), generator=g) + 0.25
    S[:, :, V - 1] = 0.0
    rows = [7, 0, 7]  # the zero-stake row, a duplicate
    got, hist = check(variant, params(variant, liquid, 2), W, S, rows)
    assert got.extra["w_path"] == path and not bool(torch.isnan(hist.B_hist).any())
    # the widened run holds the same bits
    wide = engine.run(variant, params(variant, liquid, 2), Wf.to(torch.float32), S, want_hist=True)
    assert torch.equal(bits(got.B_rows), bits(gather(wide.B_hist, rows)))


@pytest.mark.parametrize("variant,liquid", GROUP)
def test_combined_outputs(variant, liquid):
    W, S = inputs(6, 2, 5, 8)
    prm = params(variant, liquid, 2)
    ref = engine.run(variant, prm, W, S, want_hist=True)
    # both histories
    r = engine.run(variant, prm, W, S, want_hist=True, watch_rows=ROWS)
    assert r.extra["rows_path"] == "native" and r.B_hist is not None
    assert torch.equal(bits(r.B_hist), bits(ref.B_hist)) and torch.equal(bits(r.B_rows), bits(gather(ref.B_hist, ROWS)))
    # a column list beside the row list
    r = engine.run(variant, prm, W, S, watch=[7, 0], watch_rows=ROWS)
    assert r.extra["rows_path"] == "native" and r.extra["watch_path"] == "native" and r.B_hist is None
    assert torch.equal(bits(r.B_rows), bits(gather(ref.B_hist, ROWS)))
    assert torch.equal(bits(r.B_watch), bits(ref.B_hist[..., [7, 0]]))
    assert r.watch_cols == (7, 0) and r.watch_rows == tuple(ROWS)
    # the bond movement beside the row list
    r = engine.run(variant, prm, W, S, want_move=True, watch_rows=ROWS)
    assert r.extra["rows_path"] == "native" and r.extra["move_path"] == "native" and r.B_hist is None
    assert torch.equal(bits(r.B_rows), bits(gather(ref.B_hist, ROWS)))
    assert torch.equal(bits(r.B_move), bits(engine.move_from_history(ref.B_hist, None)))
    for name in ("Dn", "C", "I", "B_final"):
        assert torch.equal(bits(getattr(r, name)), bits(getattr(ref, name))), name
    # ... and where the movement is reduced from a dense history, the rows are gathered from it
    r = engine.run(variant, prm, W, S, want_move=True, want_hist=True, watch_rows=ROWS)
    assert r.extra["move_path"] == "dense" and r.extra["rows_path"] == "dense"
    assert torch.equal(bits(r.B_rows), bits(gather(ref.B_hist, ROWS)))


@pytest.mark.parametrize("variant,liquid", GROUP)
def test_streamed_validators(variant, liquid):
    W, S = inputs(3, 1, 1030, 8)  # above 1024 validators: the streamed phase 1
    check(variant, params(variant, liquid, 1), W, S, [0, 1029, 1024])


@pytest.mark.parametrize("variant,liquid", GROUP)
def test_graph_replays_and_follows_the_list_in_place(variant, liquid):
    W, S = inputs(6, 2, 5, 8)
    prm = params(variant, liquid, 2)
    hist = engine.run(variant, prm, W, S, want_hist=True).B_hist
    dev = hist.device
    lst = torch.tensor(ROWS, dtype=torch.int32, device=dev)
    direct = engine.run(variant, prm, W, S, watch_rows=lst)
    assert direct.extra["watch_rows"] is lst
    g = engine.RunGraph(variant, prm, W, S, watch_rows=lst)
    try:
        assert g.result.extra["watch_rows"] is lst and g.result.extra["rows_path"] == "native"
        for _ in range(2):
            g.result.B_rows.fill_(float("nan"))
            r = g.launch()
            torch.cuda.synchronize()
            assert torch.equal(bits(r.B_rows), bits(direct.B_rows))
            assert torch.equal(bits(r.B_rows), bits(gather(hist, ROWS)))
            assert torch.equal(bits(r.Dn), bits(direct.Dn)) and torch.equal(bits(r.B_final), bits(direct.B_final))
        lst.copy_(torch.tensor([2, 3, 0], dtype=torch.int32))
        r = g.launch()
        torch.cuda.synchronize()
        assert torch.equal(bits(r.B_rows), bits(gather(hist, [2, 3, 0])))
    finally:
        g.close()


def test_graph_refuses_what_is_not_native():
    W, S = inputs(6, 2, 6, 8)
    prm = [engine.make_params(Y1, config(True, i)) for i in range(2)]
    with pytest.raises(engine.EngineError, match="watch_rows"):
        engine.RunGraph(Y1, prm, W, S, watch_rows=[5, 0])
    with pytest.raises(engine.EngineError, match="watch_rows"):
        engine.RunGraph(Y3, params(Y3, False, 3), W[:, :1], S[:, :1], shared_inputs=True, watch_rows=[5, 0])


@pytest.mark.parametrize("variant", [RUST, Y1, Y2], ids=["yuma0", "yuma1", "yuma2"])
def test_fallback_gathers_a_dense_history(variant):
    W, S = inputs(6, 2, 6, 8)
    prm = [engine.make_params(variant, config(variant == Y1, i)) for i in range(2)]
    assert not engine.rows_native(variant, 2, 6, 6, 8, 3)
    check(variant, prm, W, S, [5, 0, 5], native=False)
    check(variant, prm, W, S, [5, 0, 5], native=False, hist_stride=2)
    both = engine.run(variant, prm, W, S, want_hist=True, watch_rows=[5, 0, 5])
    assert both.extra["rows_path"] == "dense" and both.B_hist is not None
    assert torch.equal(bits(both.B_rows), bits(gather(both.B_hist, [5, 0, 5])))


def test_shared_inputs_and_single_call_fall_back_too():
    W, S = inputs(6, 1, 6, 8)
    prm = params(Y3, False, 3)
    got = engine.run(Y3, prm, W, S, shared_inputs=True, watch_rows=[5, 0])
    hist = engine.run(Y3, prm, W, S, shared_inputs=True, want_hist=True)
    assert got.extra["rows_path"] == "dense" and got.B_hist is None
    assert torch.equal(bits(got.B_rows), bits(gather(hist.B_hist, [5, 0])))
    W, S = inputs(1, 2, 6, 8)
    check(Y3, params(Y3, False, 2), W, S, [5, 0], native=False, single_call=True)


@pytest.mark.parametrize("variant,liquid,version", [
    pytest.param(Y3, False, "Yuma 3.1 (Rhef+reset)", id="yuma31"),
    pytest.param(Y4, True, "Yuma 4 (Rhef+relative bonds) - liquid alpha on", id="yuma4-liquid"),
])
def test_oracle_at_the_watched_rows(variant, liquid, version):
    """The oracle's epoch loop, the params' reset applied by hand between its
    epochs (the rule of the engine's record: the column zeroed before epoch T,
    Yuma 4 only if the previous epoch's consensus of that miner is 0)."""
    E, V, M, rows, T, col = 8, 5, 8, [3, 0, 2], 3, 5
    always = variant == Y3
    W, S = inputs(E, 1, V, M, zero_col=None if always else (T - 1, col))
    S[:, :, V - 1] = 0.125  # (the oracle comparison keeps every validator staked)
    cfg = config(liquid, 0)
    mode = engine.RESET_ALWAYS if always else engine.RESET_IF_ZERO_CONSENSUS
    prm = [engine.make_params(variant, cfg, reset_mode=mode, reset_epoch=T, reset_index=col, n_miners=M, n_epochs=E)]
    got = engine.run(variant, prm, W, S, watch_rows=rows)
    okey, B, C_prev, ref = orc.VERSIONS[version][0], None, None, []
    for t in range(E):
        if B is not None and t == T and (always or C_prev[col] == 0.0):
            B = B.copy()
            B[:, col] = 0.0
        res = orc.epoch(okey, W[t, 0].numpy(), S[t, 0].numpy(), B, cfg)
        B, C_prev = res[orc.state_key(okey)], res["server_consensus_weight"]
        ref.append(np.array(B, copy=True))
    if not always:
        assert float(got.C[T - 1, 0, col]) == 0.0  # the conditional reset fired
    assert_close(got.B_rows[:, 0].cpu().numpy(), np.stack(ref)[:, rows, :], what="B at the watched rows")


@pytest.mark.parametrize("kw", [{}, {"bonds_every": 2}, {"dedup_inputs": True}],
                         ids=["default", "every2", "dedup"])
def test_run_simulations_bonds_validators(kw):
    versions = ("Yuma 3 (Rhef)", "Yuma 4 (Rhef+relative bonds) - liquid alpha on", "Yuma 1 (paper)")
    runs = [SimulationRun(case, v, YumaConfig(yuma_params=YumaParams(liquid_alpha="liquid" in v)))
            for case in builtin_cases[:2] for v in versions]
    ref = run_simulations(runs, **kw)
    got = run_simulations(runs, bonds_validators=[0, 2], **kw)
    for (d0, b0, i0), (d1, b1, i1) in zip(ref, got):
        assert d0 == d1 and len(b0) == len(b1) > 0
        for x, y in zip(b0, b1):
            assert y.shape == (2, x.shape[1])
            assert torch.equal(bits(y), bits(x[[0, 2], :]))
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(i0, i1))
