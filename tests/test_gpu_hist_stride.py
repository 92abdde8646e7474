"""Strided bond history (gpu marker): engine.run(..., hist_stride=, hist_first=)
on every bond scan that writes a history (k_bonds, k_bonds_cn, k_rust_big_*,
k_bonds_elem in its wide, 64-miner-tile and scalar shapes, k_bonds_grp), with
fp32, uint16 and shared inputs, direct and as a graph.

  * bitwise: slot j of the strided history is the dense history's slice at
    epoch hist_epochs[j], for strides whose stored epochs fall on both sides of
    the chunk boundaries (chunk_epochs = 4) and in chunks that start after
    epoch 0; every other output has the dense run's bits (a strided run takes
    the dense run's launch shape, so Dn included);
  * no stray stores: the slices around the history and a history of no slots
    keep a NaN bit pattern;
  * the oracle at the stored epochs;
  * stride 1 is the dense history;
  * run_simulations(..., bonds_every=).

Inputs are synth.weights / synth.stakes(period=3), E = 11; the shapes are
those tests/test_gpu_resume.py lists for the launch shapes that write history."""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import pytest
import torch

from conftest import assert_close
from oracle import yuma_oracle as orc

pytestmark = pytest.mark.gpu

from yuma_simulation._internal import engine, synth  # noqa: E402
from yuma_simulation._internal.cases import cases as builtin_cases  # noqa: E402
from yuma_simulation._internal.simulation_utils import SimulationRun, run_simulations  # noqa: E402
from yuma_simulation._internal.yumas import (  # noqa: E402
    SimulationHyperparameters,
    YumaConfig,
    YumaParams,
)

RUST, Y1, Y2, Y3, Y4 = (engine.VARIANT_RUST, engine.VARIANT_YUMA1, engine.VARIANT_YUMA2,
                        engine.VARIANT_YUMA3, engine.VARIANT_YUMA4)
NAME = {RUST: "rust", Y1: "yuma1", Y2: "yuma2", Y3: "yuma3", Y4: "yuma4"}
VERSION = {RUST: "Yuma 0 (subtensor)", Y1: "Yuma 1 (paper)", Y2: "Yuma 2 (Adrian-Fish)",
           Y3: "Yuma 3 (Rhef)", Y4: "Yuma 4 (Rhef+relative bonds)"}
ALL5 = (RUST, Y1, Y2, Y3, Y4)
E = 11
CHUNK = 4  # chunks [0,4) [4,8) [8,11): stored epochs on both sides of a boundary, chunks with t0 != 0
# (stride, first): first None = stride - 1
STRIDES = ((3, None), (4, 0), (5, 7), (11, 10))
RESET_EPOCH = 5  # stored by none of (4, 0), (5, 7), (11, 10)
SENTINEL = 0x7FC0DEAD  # a quiet NaN's bits, as int32


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "gpu tests need a ROCm GPU"
    engine.load_library()
    yield
    torch.cuda.empty_cache()


@dataclass(frozen=True)
class Case:
    id: str
    variant: int
    N: int
    V: int
    M: int
    liquid: bool = False
    kind: str = "run"  # run | sweep | u16 | graph
    reset: bool = False  # Yuma 3, reset_mode ALWAYS at RESET_EPOCH
    # the bond scan the case is there to reach under a stride, as tests/test_scan_plan_host.py spells a plan
    # (reached()): kernel or k_bonds_elem shape, then +rq +hs ... and /scalar; checked there without a GPU
    reach: str = ""


def _cases():
    c = []
    # k_bonds RC_256_1 / RC_256_4 (column-normalised, <= 64 validators), the
    # 64-miner-tile history scan for Yuma 3 / 4
    for V in (16, 40):
        c += [Case(f"small{V}-{NAME[v]}", v, 2, V, 132,
                   reach="tile_hist+hs" if v in (Y3, Y4) else f"k_bonds<256,{1 if V == 16 else 4}>+hs") for v in ALL5]
    # k_bonds_cn at 1, 2, 4, 8 rows per lane, a half-filled last strip
    c += [Case(f"strip-V{V}", RUST, 2, V, 72, reach=f"k_bonds_cn<{rows}>+rq+hs")
          for V, rows in ((100, 1), (200, 2), (384, 4), (1000, 8))]
    # k_bonds_elem 512 x 1024, second column block 4 miners wide
    c += [Case(f"widehist-{NAME[v]}", v, 2, 70, 1028, liquid=v == Y4,
               reach="wide+rq+hs" if v in (Y1, Y2) else "wide+hs") for v in (Y1, Y2, Y3, Y4)]
    # k_bonds_elem R = 2 on 64-miner tiles
    c += [Case(f"tilehist-{NAME[v]}", v, 2, 70, 260, reach="tile_hist+hs") for v in (Y1, Y2, Y3, Y4)]
    # the VEC = false forms (M % 4 != 0): k_bonds, and the scalar one-row scan's history
    c += [Case(f"scalar-hist-{NAME[v]}", v, 1, 70, 262,
               reach="k_bonds<256,16>+hs/scalar" if v == RUST else "flat1+hs/scalar") for v in ALL5]
    # k_bonds_grp: one full group of 4 scenarios and one of 2
    c += [Case(f"sweep-hist-{NAME[v]}", v, 6, 70, 260, kind="sweep", reach="k_bonds_grp+rq+hs+hist") for v in (Y3, Y4)]
    # k_rust_big_ema / k_rust_big_norm, the element-wise scan above 1024 validators
    c += [Case(f"bigv-{NAME[v]}", v, 1, 1100, 96, reach="k_rust_big+hs" if v == RUST else "tile_hist+hs")
          for v in (RUST, Y1, Y2, Y3)]
    # native uint16 W
    c += [Case("u16-yuma3", Y3, 2, 70, 1028, kind="u16", reach="wide+hs+u16")]
    c += [Case("graph-yuma3", Y3, 2, 64, 512, kind="graph", reach="tile_hist+hs")]
    # a reset between stored epochs, on the wide and the tile scan
    c += [Case("reset-wide-yuma3", Y3, 2, 70, 1028, reset=True, reach="wide+hs"),
          Case("reset-tile-yuma3", Y3, 2, 70, 260, reset=True, reach="tile_hist+hs")]
    return c


def plan_args(case):
    """engine.scan_plan's arguments for a case's strided runs (stride 3 from epoch 2)."""
    return (case.variant, case.N, E, case.V, case.M), dict(
        want_hist=True, hist_stride=3, shared_inputs=case.kind == "sweep", w_u16=case.kind == "u16")


# every (kernel or shape, strip rows) the list reaches: a case taken out or moved must leave this as it is
COVERED = {"k_bonds<256,1>", "k_bonds<256,4>", "k_bonds<256,16>", "k_bonds_cn<1>", "k_bonds_cn<2>", "k_bonds_cn<4>",
           "k_bonds_cn<8>", "k_rust_big", "k_bonds_grp", "wide", "tile_hist", "flat1"}


CASES = _cases()


def configs(case):
    """One configuration per scenario; the sweep mixes fixed and liquid alpha,
    two kappas and per-scenario bond parameters (as tests/test_gpu_resume.py),
    so that no two scenarios of a group hold the same bonds."""
    if case.kind == "sweep":
        return [YumaConfig(simulation=SimulationHyperparameters(kappa=0.45 + 0.1 * (i % 2), bond_penalty=0.99),
                           yuma_params=YumaParams(bond_alpha=0.05 + 0.04 * i, liquid_alpha=i % 3 == 1,
                                                  decay_rate=0.1 + 0.02 * i, capacity_alpha=0.1 + 0.01 * i))
                for i in range(case.N)]
    cfg = YumaConfig(simulation=SimulationHyperparameters(bond_penalty=0.99),
                     yuma_params=YumaParams(liquid_alpha=case.liquid))
    return [cfg] * case.N


def make_params(case, cfgs, reset=None):
    kw = {}
    if case.reset if reset is None else reset:
        kw = dict(reset_mode=engine.RESET_ALWAYS, reset_epoch=RESET_EPOCH, reset_index=case.M - 2,
                  n_miners=case.M, n_epochs=E)
    return [engine.make_params(case.variant, c, **kw) for c in cfgs]


def inputs(case, dev):
    """W [E,Nw,V,M] (host, fp32), and W / S on the device (Nw = 1 for the
    sweep; uint16 W for the u16 case)."""
    Nw = 1 if case.kind == "sweep" else case.N
    seed = 0x57D + 131 * case.V + case.M + case.variant
    W = synth.weights(seed, E, Nw, case.V, case.M)
    S = synth.stakes(seed, E, Nw, case.V, period=3)
    if case.kind == "u16":
        assert (W == W.astype(np.uint16)).all()  # synth weights are integers below 2^16 at these widths
        Wd = torch.from_numpy(W.astype(np.uint16)).to(dev)
    else:
        Wd = torch.from_numpy(W).to(dev)
    return W, S, Wd, torch.from_numpy(S).to(dev)


def bits(t):
    return t.contiguous().view(torch.int32)


def assert_strided_equals_dense(sp, dense, epochs, tag):
    assert sp.hist_epochs == epochs, tag
    assert tuple(sp.B_hist.shape) == (len(epochs),) + tuple(dense.B_hist.shape[1:]), tag
    for j, t in enumerate(epochs):
        assert torch.equal(sp.B_hist[j], dense.B_hist[t]), f"{tag}: slot {j} is not the dense history at epoch {t}"
    for k in ("B_final", "C", "I", "Dn"):  # Dn: the strided run takes the dense run's launch shape
        assert torch.equal(getattr(sp, k), getattr(dense, k)), f"{tag}: {k} differs"


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_strided_history_equals_dense_history(case):
    dev = engine.device()
    variant, N, V, M = case.variant, case.N, case.V, case.M
    params = make_params(case, configs(case))
    _, _, Wd, Sd = inputs(case, dev)
    kw = dict(want_hist=True, shared_inputs=case.kind == "sweep")
    dense = engine.run(variant, params, Wd, Sd, chunk_epochs=CHUNK, **kw)
    assert dense.hist_epochs == tuple(range(E)) and dense.B_hist.shape[0] == E
    if case.reset:  # the reset acts: epoch 5's state differs from the run without it
        plain = engine.run(variant, make_params(case, configs(case), reset=False), Wd, Sd, chunk_epochs=CHUNK, **kw)
        assert not torch.equal(plain.B_hist[RESET_EPOCH], dense.B_hist[RESET_EPOCH])
        assert torch.equal(plain.B_hist[RESET_EPOCH - 1], dense.B_hist[RESET_EPOCH - 1])

    for stride, first in STRIDES:
        epochs = engine.hist_epochs(E, stride, first)
        tag = f"{case.id} stride {stride} first {first}"
        # the history between two guard slices holding a NaN bit pattern
        buf = torch.full((len(epochs) + 2, N, V, M), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
        sp = engine.run(variant, params, Wd, Sd, chunk_epochs=CHUNK, hist_stride=stride, hist_first=first,
                        out={"B_hist": buf[1:1 + len(epochs)]}, **kw)
        torch.cuda.synchronize()
        assert sp.B_hist.data_ptr() == buf[1].data_ptr()
        if case.kind == "u16":
            assert dense.extra["w_path"] == sp.extra["w_path"] == "u16"
        assert_strided_equals_dense(sp, dense, epochs, tag)
        for g in (0, -1):
            assert bool((bits(buf[g]) == SENTINEL).all()), f"{tag}: a store outside the history"

    # one chunk (the default): the countdown runs through the whole run in one launch
    epochs = engine.hist_epochs(E, 3)
    sp = engine.run(variant, params, Wd, Sd, hist_stride=3, **kw)
    assert_strided_equals_dense(sp, dense, epochs, f"{case.id} stride 3, one chunk")

    # no slot at all (first >= E): nothing is written, the other outputs stand
    buf = torch.full((1, N, V, M), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
    sp = engine.run(variant, params, Wd, Sd, chunk_epochs=CHUNK, hist_stride=2, hist_first=E,
                    out={"B_hist": buf[:0]}, **kw)
    torch.cuda.synchronize()
    assert sp.hist_epochs == () and sp.B_hist.shape[0] == 0
    assert bool((bits(buf) == SENTINEL).all()), f"{case.id}: a store with no history slot"
    for k in ("B_final", "C", "I", "Dn"):
        assert torch.equal(getattr(sp, k), getattr(dense, k)), f"{case.id} no slots: {k} differs"

    if case.kind == "graph":
        epochs = engine.hist_epochs(E, 3)
        graph = engine.RunGraph(variant, params, Wd, Sd, want_hist=True, hist_stride=3, chunk_epochs=CHUNK)
        graph.result.B_hist.fill_(float("nan"))
        r = graph.launch()
        torch.cuda.synchronize()
        assert_strided_equals_dense(r, dense, epochs, f"{case.id} graph replay")
        graph.close()


ORACLE_CASES = [Case("tilehist-yuma3", Y3, 2, 70, 260), Case("tilehist-yuma4-liquid", Y4, 2, 70, 260, liquid=True),
                Case("strip-V200", RUST, 2, 200, 72)]


@pytest.mark.parametrize("case", ORACLE_CASES, ids=[c.id for c in ORACLE_CASES])
def test_stored_slots_match_the_oracle(case):
    dev = engine.device()
    cfgs = configs(case)
    W, S, Wd, Sd = inputs(case, dev)
    epochs = engine.hist_epochs(E, 3)
    sp = engine.run(case.variant, make_params(case, cfgs), Wd, Sd, want_hist=True, hist_stride=3, chunk_epochs=CHUNK)
    torch.cuda.synchronize()
    assert sp.B_hist.shape[0] == len(epochs) == 3
    for n in range(case.N):
        ref = orc.run(VERSION[case.variant], W[:, n], S[:, n], cfgs[n])
        np.testing.assert_array_equal(sp.C[:, n].cpu().numpy(), ref["C"], err_msg=f"{case.id} C")
        for j, t in enumerate(epochs):
            assert_close(sp.B_hist[j, n].cpu().numpy(), ref["B"][t], what=f"{case.id} scenario {n} B[{t}]")


def test_stride_one_is_the_dense_history():
    dev = engine.device()
    case = Case("tilehist-yuma3", Y3, 2, 70, 260)
    params = make_params(case, configs(case))
    _, _, Wd, Sd = inputs(case, dev)
    plain = engine.run(case.variant, params, Wd, Sd, want_hist=True)
    one = engine.run(case.variant, params, Wd, Sd, want_hist=True, hist_stride=1)
    zero = engine.run(case.variant, params, Wd, Sd, want_hist=True, hist_stride=1, hist_first=0)
    torch.cuda.synchronize()
    for r in (one, zero):
        assert r.B_hist.shape[0] == E and r.hist_epochs == tuple(range(E))
        for k in ("B_hist", "B_final", "C", "I", "Dn"):
            assert torch.equal(getattr(r, k), getattr(plain, k)), k
    assert engine.run(case.variant, params, Wd, Sd, hist_stride=3).hist_epochs is None  # no history asked for


def test_bad_history_arguments_raise():
    dev = engine.device()
    case = Case("small16-yuma3", Y3, 2, 16, 132)
    params = make_params(case, configs(case))
    _, _, Wd, Sd = inputs(case, dev)
    wrong = torch.empty(E, case.N, case.V, case.M, device=dev)
    with pytest.raises(ValueError, match="B_hist"):
        engine.run(case.variant, params, Wd, Sd, hist_stride=3, out={"B_hist": wrong})
    with pytest.raises(ValueError, match="B_hist"):
        engine.run(case.variant, params, Wd, Sd, out={"B_hist": wrong[:3]})
    with pytest.raises(ValueError):
        engine.run(case.variant, params, Wd, Sd, want_hist=True, hist_stride=0)
    with pytest.raises(ValueError):
        engine.run(case.variant, params, Wd, Sd, want_hist=True, hist_first=-1)
    with pytest.raises(ValueError, match="single_call"):
        engine.run(case.variant, params, Wd[:2], Sd[:2], want_hist=True, hist_stride=2, single_call=True)


def test_run_simulations_bonds_every():
    cfg = YumaConfig(simulation=SimulationHyperparameters(bond_penalty=0.99))
    runs = [SimulationRun(builtin_cases[0], "Yuma 1 (paper)", cfg),
            SimulationRun(builtin_cases[10], "Yuma 3 (Rhef)", cfg)]
    dense = run_simulations(runs)
    sparse = run_simulations(runs, bonds_every=3)
    for r, (div, bonds, inc), (div3, bonds3, inc3) in zip(runs, dense, sparse):
        epochs = engine.hist_epochs(len(bonds), 3)
        assert len(bonds) >= 6 and len(epochs) == len(bonds) // 3
        assert len(bonds3) == len(epochs)
        for j, t in enumerate(epochs):
            assert torch.equal(bonds3[j], bonds[t]), (r.case.name, t)
        assert div3 == div
        assert len(inc3) == len(inc) and all(torch.equal(a, b) for a, b in zip(inc3, inc))
    with pytest.raises(ValueError):
        run_simulations(runs, bonds_every=0)
