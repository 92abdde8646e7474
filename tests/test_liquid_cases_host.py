"""What tests/liquid_cases.py claims, proved from the oracle alone (no GPU).

For every (shape, family) that tests/test_gpu_liquid.py runs, `facts` reads
the oracle's sorted levels and states where the ranks of the three quantiles
land: their levels, high bytes, the lerp weight, the run of equal levels
around each rank and the distance to its edges, and the bin positions
(lane, walk position) a 64-lane, four-bins-per-lane scan of the high-byte and
low-byte histograms visits for them. The tests assert the property each
family is named for, that the table of shapes covers every family, both lerp
branches, lo == hi and both variants of the 0.99 fallback, that the oracle's
quantile equals torch.quantile and a rational restatement bit for bit, and
that moving a selected rank by one changes a or b (so a select that is off by
one cannot pass the GPU comparison)."""

from __future__ import annotations

from dataclasses import replace
from functools import lru_cache

import numpy as np
import pytest
import torch

import liquid_cases as lc
from oracle import yuma_oracle as orc

F32 = np.float32
CASES = [(M, f) for M in lc.SHAPES for f in lc.families(M)]
IDS = [f"M{M}-{f}" for M, f in CASES]
# YumaRust takes its levels in fp64: the families hold there too
RUST_CASES = [(M, f) for M in lc.OTHER_VARIANT_SHAPES for f in lc.families(M)]


@lru_cache(maxsize=None)
def facts(M: int, family: str, variant: str = "yuma4") -> dict:
    ref = lc.reference(M, variant)
    e = lc.families(M).index(family)
    s = np.sort(lc.levels(ref["C"][e]))
    out = {"sorted": s, "a": ref["ab"][e, 0], "b": ref["ab"][e, 1], "max": int(s[-1]),
           "bond_alpha": ref["bond_alpha"][e], "e": e}
    for q in lc.QS:
        lo, hi, w = lc.ranks(M, q)
        run = []
        for r in (lo, hi):
            first = int(np.searchsorted(s, s[r], "left"))
            last = int(np.searchsorted(s, s[r], "right")) - 1
            run.append((r - first, last - r))      # distance to the run's first / last element
        bins = []
        for r in (lo, hi):                          # the scan positions of the two-level select
            hb, lb = int(s[r]) >> 8, int(s[r]) & 255
            bins.append(((hb // 4, hb % 4), (lb // 4, lb % 4)))
        out[q] = {"lo": lo, "hi": hi, "w": w, "levels": (int(s[lo]), int(s[hi])),
                  "bytes": (int(s[lo]) >> 8, int(s[hi]) >> 8), "run": run, "bins": bins,
                  "value": orc.quantile((s.astype(F32) / F32(65535.0)).astype(F32), q)}
    out["eq"] = out[0.75]["value"] == out[0.25]["value"]
    return out


def check_family(M, family, f):
    q25, q75, q99 = f[0.25], f[0.75], f[0.99]
    if family in ("sparseA", "sparseB"):
        assert (f["sorted"] == 0).mean() >= 0.76
        assert q25["levels"] == q75["levels"] == (0, 0) and f["eq"]
        assert np.isfinite(f["a"]) and np.isfinite(f["b"]) and f["a"] > 0    # the 0.99 fallback, finite
        if family == "sparseA":
            assert q99["bytes"][0] == q99["bytes"][1]
        else:
            assert q99["levels"] == (255, 256) and q99["bytes"] == (0, 1)      # b1 != b0
            assert q99["run"][0][1] == 0 and q99["run"][1][0] == 0             # last of its run | first of its run
    elif family in ("flat", "zero"):
        assert f["eq"] and q99["value"] == q75["value"]                        # d == 0
        assert f["a"] == -np.inf and (np.isnan(f["b"]) or f["b"] == -np.inf)
        assert np.isnan(f["bond_alpha"]).all()
        if family == "zero":
            assert len(set(f["sorted"].tolist())) == 1
        if M == 65540:
            assert q99["levels"] == (0, 0) and np.isnan(f["b"])                # a uniform wide subnet: all zeros
            assert (f["sorted"] == 0).sum() > 65535                            # one bin counts past 16 bits
    elif family in ("straddle75", "straddle25"):
        q = q75 if family == "straddle75" else q25
        assert q["levels"] == (255, 256) and q["bytes"] == (0, 1) and q["hi"] == q["lo"] + 1
        assert not f["eq"] and np.isfinite(f["a"]) and np.isfinite(f["b"])
    elif family == "spread":
        assert len(set(f["sorted"].tolist())) >= 40
        assert not f["eq"] and np.isfinite(f["a"]) and np.isfinite(f["b"])
        for q in (q25, q75):                                                   # ranks inside runs of ties
            assert all(a + b >= (8 if M >= 900 else 1) for a, b in q["run"])
    else:
        assert family == "top"
        assert f["max"] == {1: 65535, 2: 65405, 3: 32767, 5: 28117}[M]
        assert np.isfinite(f["a"]) == (M > 1)


@pytest.mark.parametrize("M,family", CASES, ids=IDS)
def test_family_has_the_property_it_is_named_for(M, family):
    f = facts(M, family)
    check_family(M, family, f)
    for q in lc.QS:                       # (lo == hi) <=> the rank is integral, only at (M - 1) % 4 == 0
        assert (f[q]["lo"] == f[q]["hi"]) == (f[q]["w"] == 0.0)
    assert (f[0.25]["lo"] == f[0.25]["hi"]) == ((M - 1) % 4 == 0)


@pytest.mark.parametrize("M,family", RUST_CASES, ids=[f"M{M}-{f}" for M, f in RUST_CASES])
def test_family_holds_for_fp64_levels(M, family):
    check_family(M, family, facts(M, family, "rust"))


def test_inputs_are_order_independent():
    for M in lc.SHAPES:
        inp = lc.build(M)
        assert inp.W.shape == (len(inp.families), lc.V, M) and len(inp.families) <= 7
        assert (inp.W == inp.W[:, :1]).all() and (inp.W == np.floor(inp.W)).all() and inp.W.max() <= 65535
        sums = inp.W.astype(np.float64).sum(axis=2)
        assert set(np.unique(sums).tolist()) <= {0.0, float(lc.row_sum(M))}
        assert (inp.S == lc.STAKE_TOTAL // lc.V).all() and inp.S.sum(axis=1).tolist() == [lc.STAKE_TOTAL] * len(inp.families)
        assert inp.families.index("zero") > 0
        # sum(C_raw): multiples of 2^-17 below 2^7, exact in any order
        craw = np.maximum(inp.W[:, 0].astype(np.int64), 1) * ((1 << 17) // lc.row_sum(M))
        assert craw.sum(axis=1).max() < 1 << 24


def test_table_covers_every_family_and_branch():
    seen = {f for _, f in CASES}
    assert seen == set(lc.FAMILIES)
    assert set(lc.SHAPES) >= {1, 2, 3, 5, 261, 900, 2308, 2051, 65540}
    w = {(q, round(facts(M, f)[q]["w"], 2)) for M, f in CASES for q in (0.25, 0.75)}
    assert {(0.25, 0.25), (0.25, 0.75), (0.75, 0.25), (0.75, 0.75), (0.25, 0.0), (0.75, 0.5)} <= w   # both lerp forms, lo == hi
    w99 = [facts(M, f)[0.99]["w"] for M, f in CASES if f.startswith("sparse")]
    assert min(w99) < 0.5 <= max(w99)                                  # both forms on the fallback too
    for fam in ("sparseA", "sparseB"):                                 # each 0.99 variant where the loops differ
        Ms = {M for M, f in CASES if f == fam}
        assert {261, 900, 2051, 2308} <= Ms
    assert (65540, "sparseA") in CASES
    assert {M for M, f in CASES if f == "straddle75"} >= {900} and (262, "straddle25") in CASES
    # the scan positions the selected ranks visit, over the whole table
    used = {"sparseA": (0.25, 0.75, 0.99), "sparseB": (0.25, 0.75, 0.99), "flat": lc.QS, "zero": lc.QS}
    high, low = set(), set()
    for M, f in CASES:
        for q in used.get(f, (0.25, 0.75)):
            for hb, lb in facts(M, f)[q]["bins"]:
                high.add(hb)
                low.add(lb)
    for name, got in (("high byte", high), ("low byte", low)):
        assert {i for _, i in got} == {0, 1, 2, 3}, name               # every walk position
        assert len({lane for lane, _ in got if lane > 0}) >= 4, name   # lanes other than 0
    assert (63, 3) in high and (63, 3) in low                          # level 65535; level 255


@pytest.mark.parametrize("M,family", CASES, ids=IDS)
def test_quantile_equals_torch_and_rational(M, family):
    f = facts(M, family)
    C = lc.reference(M)["C"][f["e"]]
    for q in lc.QS:
        got = orc.quantile(C, q)
        want = torch.quantile(torch.from_numpy(np.array(C)), q).numpy()
        assert got.view(np.int32) == want.view(np.int32), (q, got, want)
        exact = lc.quantile_exact(f["sorted"], q)
        assert got.view(np.int32) == exact.view(np.int32), (q, got, exact)


def fit_with(C, high=None, low=None):
    """a, b of the oracle with consensus_high or _low replaced (one override
    takes the fp32 path of the quantile fit)."""
    _, a, b = orc.liquid_alpha(C, replace(lc.Config(), override_consensus_high=high, override_consensus_low=low))
    return F32(a), F32(b)


def lerp_at(s, lo, hi, w):
    a, b = (F32(F32(s[i]) / F32(65535.0)) for i in (lo, hi))
    d = F32(b - a)
    return orc.fma32(w, d, a) if abs(w) < 0.5 else orc.fma32(-d, F32(F32(1.0) - F32(w)), b)


@pytest.mark.parametrize("M,family", [c for c in CASES if c[1] in ("straddle75", "straddle25")],
                         ids=[i for i, c in zip(IDS, CASES) if c[1] in ("straddle75", "straddle25")])
def test_one_rank_off_changes_the_fit(M, family):
    """Non-tie families: either selected rank, moved by one either way, gives another a or b."""
    f = facts(M, family)
    C = lc.reference(M)["C"][f["e"]]
    q = 0.75 if family == "straddle75" else 0.25
    lo, hi, w = f[q]["lo"], f[q]["hi"], F32(f[q]["w"])
    key = "high" if q == 0.75 else "low"
    base = fit_with(C, **{key: float(lerp_at(f["sorted"], lo, hi, w))})
    assert base[0].view(np.int32) == f["a"].view(np.int32) and base[1].view(np.int32) == f["b"].view(np.int32)
    for dlo, dhi in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        moved = fit_with(C, **{key: float(lerp_at(f["sorted"], lo + dlo, hi + dhi, w))})
        assert moved != base, (dlo, dhi)
    # floor in place of ceil for the upper rank is another value too
    assert fit_with(C, **{key: float(lerp_at(f["sorted"], lo, lo, w))}) != base


@pytest.mark.parametrize("M", [2, 3, 5])
def test_one_rank_off_changes_the_fit_in_top(M):
    """`top` (the other non-tie family): every step of a selected rank that
    lands on another level gives another a or b, and each of the two quantiles
    has such a step. (Where lo == hi the weight is 0 and the two move
    together; a step inside a pair of equal levels selects the same value.)"""
    f = facts(M, "top")
    C = lc.reference(M)["C"][f["e"]]
    s = f["sorted"]
    base = (f["a"], f["b"])
    for q, key in ((0.25, "low"), (0.75, "high")):
        lo, hi, w = f[q]["lo"], f[q]["hi"], F32(f[q]["w"])
        taken = lerp_at(s, lo, hi, w)
        assert fit_with(C, **{key: float(taken)}) == base
        moves = ((-1, 0), (1, 0), (0, -1), (0, 1)) if lo != hi else ((-1, -1), (1, 1))
        changed = 0
        for dlo, dhi in moves:
            if not (0 <= lo + dlo <= hi + dhi < M):
                continue
            if (s[lo + dlo], s[hi + dhi]) != (s[lo], s[hi]):
                assert fit_with(C, **{key: float(lerp_at(s, lo + dlo, hi + dhi, w))}) != base, (q, dlo, dhi)
                changed += 1
        assert changed >= 1, q


def test_other_lerp_form_changes_the_fit():
    """The two forms of the lerp are the same real number and differ in fp32
    only where b - a rounds: levels more than a factor of two apart. `top` at
    M = 2 has them, with w = 0.25 (first form) and w = 0.75 (second form)."""
    f = facts(2, "top")
    C = lc.reference(2)["C"][f["e"]]
    s = f["sorted"]
    a, b = (F32(F32(x) / F32(65535.0)) for x in s)
    d = F32(b - a)
    assert np.float64(b) - np.float64(a) != np.float64(d)
    base = (f["a"], f["b"])
    for q, key in ((0.25, "low"), (0.75, "high")):
        w = F32(f[q]["w"])
        assert (q, float(w)) in ((0.25, 0.25), (0.75, 0.75))
        taken = lerp_at(s, 0, 1, w)
        other = orc.fma32(-d, F32(F32(1.0) - w), b) if abs(w) < 0.5 else orc.fma32(w, d, a)
        assert taken.view(np.int32) == f[q]["value"].view(np.int32) and other != taken
        assert fit_with(C, **{key: float(taken)}) == base
        assert fit_with(C, **{key: float(other)}) != base, q


def test_fallback_rank_off_by_one_changes_the_fit():
    """sparseB: the 0.99 ranks sit on a run's last and the next run's first
    element, so one step across the edge changes consensus_high."""
    for M, family in CASES:
        if family != "sparseB":
            continue
        f = facts(M, family)
        C = lc.reference(M)["C"][f["e"]]
        lo, hi, w = f[0.99]["lo"], f[0.99]["hi"], F32(f[0.99]["w"])
        # (high == low == 0 here: give the fallback's value as consensus_high against low = 0)
        base = fit_with(C, high=float(lerp_at(f["sorted"], lo, hi, w)))
        assert base[0].view(np.int32) == f["a"].view(np.int32) and base[1].view(np.int32) == f["b"].view(np.int32)
        assert fit_with(C, high=float(lerp_at(f["sorted"], lo + 1, hi, w))) != base
        assert fit_with(C, high=float(lerp_at(f["sorted"], lo, hi - 1, w))) != base


def test_tie_families_reach_a_run_edge():
    """Tie families: the ranks the fit reads lie inside runs of equal levels
    (printed with the distance to either edge); per family at least one shape
    has a rank ON the first or last element of its run, where an off-by-one in
    the histogram scan shows."""
    reads = {"sparseA": lc.QS, "sparseB": lc.QS, "flat": lc.QS, "spread": (0.25, 0.75)}
    edge = {fam: [] for fam in lc.TIE_FAMILIES}
    for M, family in CASES:
        if family not in reads:
            continue
        f = facts(M, family)
        for q in reads[family]:
            for which, r, (before, after) in zip(("lo", "hi"), (f[q]["lo"], f[q]["hi"]), f[q]["run"]):
                print(f"[liquid cases] M {M} {family} q {q} {which} rank {r}: level {int(f['sorted'][r])}, "
                      f"{before} after its run's first element, {after} before its last")
                if q != 0.99 or family == "flat":  # (the 0.99 ranks of a small sparse shape may be singles)
                    assert before + after >= 1, (M, family, q)      # a run of ties, not a single
                if min(before, after) == 0:
                    edge[family].append((M, q, which))
    for fam, hits in edge.items():
        assert hits, f"{fam}: no shape has a rank on a run's edge"
