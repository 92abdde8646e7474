"""The liquid-alpha block on the GPU (gpu marker): the two-level quantile
select, the decision ladder and the logistic fit of k_quantise<256>, and
k_liquid<256> on the miner-column-sharded path, against the oracle.

Inputs are tests/liquid_cases.py's: one family of quantisation levels per
epoch, order-independent, so C, the levels, consensus_high / _low, a and b
have one correct value each (tests/test_liquid_cases_host.py proves the
families and that a rank off by one changes a or b). Every case is V = 4 and
one run of E = the number of families the shape admits.

Per run, against oracle.run and the oracle's liquid-alpha block:
  * C bit-equal;
  * alpha_ab bit-equal to the oracle's fp32 a, b, infinite with the same sign
    where the oracle's is, NaN where it is NaN. Derived, not measured:
    cl - ch, 1 / d, inv * ln_num and ln_low + a * cl are single IEEE fp32
    operations of a library built with -ffp-contract=off and IEEE division,
    and the oracle restates them one rounding each;
  * bond_alpha within conftest.RTOL (only powf separates the two sides), its
    NaN pattern equal; where the unclamped alpha lies outside
    [alpha_low, alpha_high] by more than RTOL, bit-equal to 1 - alpha_low or
    1 - alpha_high;
  * Dn, I, B_hist, B_final within the suite's tolerance, NaN and inf patterns
    equal (assert_close enforces that).
The override ladder (six scenarios, per-scenario and shared inputs), the
sharded path (k_liquid over every shard's levels, Mq != M), RunGraph, a
chunked run and an input schedule are bit-equal to the runs they restate
(the sharded run's NaN bonds up to the sign bit of the NaN: see value_bits)."""

from __future__ import annotations

import time

import numpy as np
import pytest
import torch

import liquid_cases as lc
from conftest import RTOL, assert_close

pytestmark = pytest.mark.gpu

from yuma_simulation._internal import engine, wide  # noqa: E402
from yuma_simulation._internal.yumas import SimulationHyperparameters, YumaConfig, YumaParams  # noqa: E402

F32 = np.float32
VARIANT = {"yuma4": engine.VARIANT_YUMA4, "yuma1": engine.VARIANT_YUMA1, "yuma2": engine.VARIANT_YUMA2,
           "rust": engine.VARIANT_RUST}
WANT = ("bond_alpha", "alpha_ab")
RUNS = [(M, "yuma4") for M in lc.SHAPES] + [(M, v) for v in ("yuma1", "yuma2", "rust") for M in lc.OTHER_VARIANT_SHAPES]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "gpu tests need a ROCm GPU"
    engine.load_library()
    t0 = time.perf_counter()
    yield
    torch.cuda.empty_cache()
    print(f"[liquid] tests/test_gpu_liquid.py: {time.perf_counter() - t0:.1f} s in all")


def yconfig(c: lc.Config) -> YumaConfig:
    return YumaConfig(
        simulation=SimulationHyperparameters(kappa=c.kappa, bond_penalty=c.bond_penalty,
                                             consensus_precision=c.consensus_precision),
        yuma_params=YumaParams(bond_alpha=c.bond_alpha, liquid_alpha=c.liquid_alpha, alpha_high=c.alpha_high,
                               alpha_low=c.alpha_low, decay_rate=c.decay_rate, capacity_alpha=c.capacity_alpha,
                               override_consensus_high=c.override_consensus_high,
                               override_consensus_low=c.override_consensus_low))


def params(variant: str, c: lc.Config = lc.Config()):
    return engine.make_params(VARIANT[variant], yconfig(c))


def device_inputs(M: int, epochs=None):
    inp = lc.build(M)
    idx = list(range(len(inp.families))) if epochs is None else list(epochs)
    dev = engine.device()
    return (torch.from_numpy(inp.W[idx][:, None].copy()).to(dev),   # [E, 1, V, M]
            torch.from_numpy(inp.S[idx][:, None].copy()).to(dev))


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


def value_bits(t: torch.Tensor) -> torch.Tensor:
    """bits() with every NaN as one pattern, for the bond state of the `flat`
    and `zero` epochs alone: there the sharded and the whole run can give the
    NaN bonds opposite sign bits (0xffc00000 against 0x7fc00000, measured on
    B_final; IEEE 754 leaves the sign of a NaN result open). The NaNs have to
    be the same elements; every number is compared with bits()."""
    return torch.where(torch.isnan(t), torch.full_like(bits(t), 0x7FC00000), bits(t))


def same_bits(x, y, tag, liquid=None):
    """Two engine runs, bit for bit (bond_alpha of the liquid scenarios only:
    the engine writes it for those alone)."""
    pairs = [("Dn", x.Dn, y.Dn), ("C", x.C, y.C), ("I", x.I, y.I), ("B_final", x.B_final, y.B_final),
             ("alpha_ab", x.extra["alpha_ab"], y.extra["alpha_ab"])]
    if x.B_hist is not None and y.B_hist is not None:
        pairs.append(("B_hist", x.B_hist, y.B_hist))
    for name, a, b in pairs:
        assert torch.equal(bits(a), bits(b)), f"{tag}: {name} differs"
    N = x.C.shape[1]
    for n in range(N):
        if liquid is None or liquid[n]:
            assert torch.equal(bits(x.extra["bond_alpha"][:, n]), bits(y.extra["bond_alpha"][:, n])), \
                f"{tag}: bond_alpha of scenario {n} differs"


def check_ab(got: np.ndarray, want: np.ndarray, tag: str):
    """alpha_ab [E, 2] against the oracle's fp32 a, b: equal bits, NaN where NaN."""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    print(f"[liquid] {tag}: a, b = {got.tolist()} (oracle {want.tolist()})")
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{tag}: alpha_ab NaN pattern {got.tolist()} against {want.tolist()}"
    assert np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan]), \
        f"{tag}: alpha_ab {got.tolist()} is not the oracle's {want.tolist()}"


def check_against_oracle(res, n: int, ref: dict, c: lc.Config, tag: str):
    """Scenario n of an engine run against lc.reference (see the module docstring)."""
    C = res.C[:, n].cpu().numpy()
    bad = np.argwhere(C != ref["C"])
    assert bad.size == 0, f"{tag}: C differs at (epoch, column) {bad[:8].tolist()} ({len(bad)} in all)"
    if c.liquid_alpha:
        check_ab(res.extra["alpha_ab"][:, n].cpu().numpy(), ref["ab"], tag)
        ba = res.extra["bond_alpha"][:, n].cpu().numpy()
        assert_close(ba, ref["bond_alpha"], what=f"{tag} bond_alpha")
        lo, hi = np.float64(F32(c.alpha_low)), np.float64(F32(c.alpha_high))
        with np.errstate(invalid="ignore"):
            below, above = ref["alpha"] < lo * (1 - RTOL), ref["alpha"] > hi * (1 + RTOL)
        one = F32(1.0)
        assert (ba[below].view(np.int32) == F32(one - F32(c.alpha_low)).view(np.int32)).all(), f"{tag}: clamp at alpha_low"
        assert (ba[above].view(np.int32) == F32(one - F32(c.alpha_high)).view(np.int32)).all(), f"{tag}: clamp at alpha_high"
        print(f"[liquid] {tag}: {int(below.sum())} alphas clamped low, {int(above.sum())} high, "
              f"{int(np.isnan(ref['alpha']).sum())} NaN, of {ba.size}")
    assert_close(res.Dn[:, n].cpu().numpy(), ref["Dn"], what=f"{tag} Dn")
    assert_close(res.I[:, n].cpu().numpy(), ref["I"], what=f"{tag} I")
    if res.B_hist is not None:
        assert_close(res.B_hist[:, n].cpu().numpy(), ref["B"], what=f"{tag} B_hist")
    assert_close(res.B_final[n].cpu().numpy(), ref["B"][-1], what=f"{tag} B_final")


_PLAIN: dict = {}


def plain_run(M: int, variant: str = "yuma4"):
    """The whole-shape run with a history (once per shape and variant)."""
    if (M, variant) not in _PLAIN:
        W, S = device_inputs(M)
        res = engine.run(VARIANT[variant], [params(variant)], W, S, want_hist=True, want=WANT)
        torch.cuda.synchronize()
        _PLAIN[M, variant] = res
    return _PLAIN[M, variant]


@pytest.mark.parametrize("M,variant", RUNS, ids=[f"M{M}-{v}" for M, v in RUNS])
def test_run_equals_the_oracle(M, variant):
    res = plain_run(M, variant)
    assert res.C.shape == (len(lc.families(M)), 1, M)
    check_against_oracle(res, 0, lc.reference(M, variant), lc.Config(), f"M {M} {variant} {lc.families(M)}")


# ---------------------------------------------------------------------------
# the override ladder
# ---------------------------------------------------------------------------
def level(k: int) -> float:
    """A level as the Python float an override carries."""
    return float(F32(F32(k) / F32(65535.0)))


def ladder(M: int):
    """(epochs, six configurations). consensus_low of the sparse epochs is
    level 0, so `override_consensus_high=0.0` alone meets it: high == low in
    fp32 through an override. 255 | 256 are levels of the sparseB epoch."""
    fams = lc.families(M)
    epochs = tuple(fams.index(f) for f in ("sparseA", "sparseB", "straddle75" if "straddle75" in fams else "spread"))
    base = lc.Config()
    return epochs, [
        lc.with_overrides(base, liquid=False),
        base,
        lc.with_overrides(base, high=level(0)),
        lc.with_overrides(base, low=level(256)),
        lc.with_overrides(base, high=level(255), low=level(255)),
        lc.with_overrides(base, high=level(256), low=level(5)),
    ]


@pytest.mark.parametrize("M", [900, 2308])
def test_override_ladder(M):
    epochs, cfgs = ladder(M)
    prm = [params("yuma4", c) for c in cfgs]
    modes = [p.liquid_mode for p in prm]
    assert modes == [engine.LIQUID_OFF] + [engine.LIQUID_QUANTILE] * 4 + [engine.LIQUID_CONST_AB]
    assert [p.override_flags for p in prm[1:5]] == [0, engine.OVR_HIGH, engine.OVR_LOW,
                                                    engine.OVR_HIGH | engine.OVR_LOW | engine.OVR_FORCE_Q99]
    W, S = device_inputs(M, epochs)
    E, N, V = len(epochs), len(cfgs), lc.V
    own = engine.run(VARIANT["yuma4"], prm, W.expand(E, N, V, M).contiguous(), S.expand(E, N, V).contiguous(),
                     want_hist=True, want=WANT)
    shared = engine.run(VARIANT["yuma4"], prm, W, S, want_hist=True, want=WANT, shared_inputs=True)
    torch.cuda.synchronize()
    liquid = [c.liquid_alpha for c in cfgs]
    same_bits(own, shared, f"M {M} ladder, per-scenario against shared inputs", liquid=liquid)
    for res, how in ((own, "per-scenario"), (shared, "shared")):
        for n, c in enumerate(cfgs):
            ref = lc.reference(M, "yuma4", c, epochs)
            check_against_oracle(res, n, ref, c, f"M {M} ladder {how} scenario {n}")
    # high-only met the selected low: the fallback's value, not the override, made the fit
    fell = lc.reference(M, "yuma4", cfgs[2], epochs)["ab"]
    assert np.array_equal(fell[:2], lc.reference(M, "yuma4", cfgs[1], epochs)["ab"][:2]) and np.isfinite(fell).all()


# ---------------------------------------------------------------------------
# the sharded path: k_liquid over every shard's levels
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("M,counts", [(2308, (2, 3, 5)), (65540, (2, 7))], ids=["M2308", "M65540"])
def test_sharded_run_equals_the_unsharded(M, counts):
    """C, alpha_ab and bond_alpha of every epoch, and the bond state after
    every epoch (B_hist), by bits. The epochs before `flat` have finite bonds:
    there every element is compared as a number, bit for bit, and a second
    sharded run over those epochs alone ends on a finite B_final that is
    compared the same way. From `flat` on the bonds are NaN in both runs; only
    there, and only for the bond state, value_bits stands in for bits."""
    whole = plain_run(M)
    W, S = device_inputs(M)
    fams = lc.families(M)
    n_fin = fams.index("flat")                       # the epochs before it have finite bonds
    assert n_fin >= 1 and bool(torch.isfinite(whole.B_hist[:n_fin]).all())
    assert bool((whole.B_hist[n_fin - 1] != 0).any()) and bool(torch.isnan(whole.B_final).all())
    Wf, Sf = device_inputs(M, range(n_fin))
    for n_shards in counts:
        cols = wide.column_ranges(M, n_shards)
        assert len(cols[-1]) % wide.TILE and len({len(c) for c in cols}) > 1   # a partly filled last shard
        ws = wide.run_wide_local(VARIANT["yuma4"], [params("yuma4")], W, S, n_shards, want=WANT, want_hist=True)
        fin = wide.run_wide_local(VARIANT["yuma4"], [params("yuma4")], Wf, Sf, n_shards, want=WANT)
        torch.cuda.synchronize()
        tag = f"M {M}, {n_shards} shards"
        assert all(c.shape[2] < M for c in ws.C)
        hist = torch.cat(ws.B_hist, dim=3)
        for name, got, ref in (("C", torch.cat(ws.C, dim=2), whole.C),
                               ("bond_alpha", torch.cat(ws.extra["bond_alpha"], dim=2), whole.extra["bond_alpha"]),
                               ("B_hist of the finite epochs", hist[:n_fin], whole.B_hist[:n_fin]),
                               ("B_final of the finite epochs", torch.cat(fin.B_final, dim=2), whole.B_hist[n_fin - 1]),
                               ("bond_alpha of the finite epochs", torch.cat(fin.extra["bond_alpha"], dim=2),
                                whole.extra["bond_alpha"][:n_fin])):
            assert torch.equal(bits(got), bits(ref)), f"{tag}: {name} differs from the unsharded run"
        for name, got, ref in (("B_hist", hist, whole.B_hist), ("B_final", torch.cat(ws.B_final, dim=2), whole.B_final)):
            assert torch.equal(value_bits(got), value_bits(ref)), f"{tag}: {name} differs from the unsharded run"
        for i, ab in enumerate(ws.extra["alpha_ab"]):
            assert torch.equal(bits(ab), bits(whole.extra["alpha_ab"])), f"{tag}: alpha_ab of shard {i}"
            assert torch.equal(bits(fin.extra["alpha_ab"][i]), bits(whole.extra["alpha_ab"][:n_fin])), tag
        check_ab(ws.extra["alpha_ab"][-1][:, 0].cpu().numpy(), lc.reference(M)["ab"], tag)


# ---------------------------------------------------------------------------
# the other run paths
# ---------------------------------------------------------------------------
def test_graph_chunked_and_scheduled_runs_equal_the_plain_run():
    M = 900
    whole = plain_run(M)
    W, S = device_inputs(M)
    prm = [params("yuma4")]
    g = engine.RunGraph(VARIANT["yuma4"], prm, W, S, want_hist=True, want=WANT)
    try:
        r = g.launch()
        torch.cuda.synchronize()
        same_bits(r, whole, "RunGraph")
    finally:
        g.close()
    chunked = engine.run(VARIANT["yuma4"], prm, W, S, want_hist=True, want=WANT, chunk_epochs=2)
    torch.cuda.synchronize()
    same_bits(chunked, whole, "chunk_epochs=2")
    fams = lc.families(M)
    sched = [fams.index("sparseB"), fams.index("straddle75")] * 3 + [fams.index("flat")]
    got = engine.run(VARIANT["yuma4"], prm, W, S, sched=sched, want_hist=True, want=WANT)
    ref = engine.run(VARIANT["yuma4"], prm, W[sched].contiguous(), S[sched].contiguous(), want_hist=True, want=WANT)
    torch.cuda.synchronize()
    same_bits(got, ref, f"sched {sched}")
    check_against_oracle(got, 0, lc.reference(M, "yuma4", lc.Config(), tuple(sched)), lc.Config(), f"sched {sched}")
