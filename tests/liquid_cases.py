"""Inputs with a prescribed distribution of quantisation levels, for the
liquid-alpha block (quantile select, logistic fit, bond_alpha).

Host side only (numpy and oracle/, no GPU, no engine). Used by
tests/test_liquid_cases_host.py, which proves from the oracle what is claimed
here, and by tests/test_gpu_liquid.py, which runs the engine on these inputs.

Inputs (`build`) are order-independent by construction:

  * weights: every validator gives the same integer row, entries <= 65535,
    row sum 2^17 (2^15 where M <= 2: two entries <= 65535 cannot reach 2^17),
    so Wn = W / rowsum exactly and rowsum + 1e-6 == rowsum in fp32;
  * stakes: V equal integer raw stakes totalling 2^20, so every subset sum of
    the normalised stakes is exact.

Every validator agrees, so the consensus of column m is the grid point
max(w[m], 1) / 2^17 (2^15), sum(C_raw) is a sum of multiples of 2^-17 below
2^7, exact in any order, and C, the levels, consensus_high / _low, a and b
have one correct value each. A column of weight 0 and a column of weight 1
have the same consensus: the lowest grid point.

One family per epoch (`FAMILIES`, `families(M)`: what a shape admits), the
columns in a fixed pseudo-random order (the sorted order is never the memory
order). Ranks below are 0-based positions in the sorted levels; a quantile q
reads lo = int(rank), hi = ceil(rank), rank = fp32(q) * (M - 1) in fp32.

  sparseA    >= 76 % of the columns at weight 0 (level 0), the others rising:
             consensus_high == consensus_low == 0, the 0.99 fallback with
             finite a, b; both 0.99 ranks in one high byte
  sparseB    the same, the 0.99 ranks on levels 255 | 256 (two high bytes,
             lo on the last element of its run, hi on the first of its run)
  flat       every column equal, the remainder of the row sum on one column
             that no rank reaches: high == low == q99, d == 0, a = -inf,
             b = NaN, every bond_alpha NaN
  zero       an all-zero weight epoch (never the first): every level equal
             again, R.sum() == 0 and P == 0, NaN alphas on a bond state
  straddle75 the 0.75 ranks on levels 255 | 256
  straddle25 the 0.25 ranks on levels 255 | 256
  spread     weights base * (1 + m % 97): 40+ distinct levels in long tie runs
  top        M = 1: level 65535; M = 2, 3, 5: a few levels far apart, in high
             bytes 0, 18, 109, 127, 255; at M = 2 each quantile's other lerp
             form would round to another value

What cannot be built: the levels of a slice total at most 65535, so a rank r
can sit on level 256 only while (M - r) * 256 <= 65535. The 0.75 ranks reach
255 | 256 up to M ~ 1000, the 0.25 ranks up to M ~ 340 (and need lo != hi,
(M - 1) % 4 != 0: M = 262), the 0.99 ranks up to M ~ 25000. For the same
reason no slice holds levels in 30 distinct high bytes (256 * (0 + ... + 29)
= 111360 > 65535); `spread` covers many low bytes instead, and the high bytes
come from `top`, `flat` and `zero` on the small shapes (level ~ 65535 / M).
"""

from __future__ import annotations

import math
from dataclasses import dataclass, replace
from fractions import Fraction
from functools import lru_cache

import numpy as np

from oracle import yuma_oracle as orc

F32 = np.float32
V = 4
STAKE_TOTAL = 1 << 20
QS = (0.25, 0.75, 0.99)
FAMILIES = ("sparseA", "sparseB", "flat", "straddle75", "straddle25", "spread", "top", "zero")
TIE_FAMILIES = ("sparseA", "sparseB", "flat", "spread")  # the selected ranks lie in runs of equal levels

# The shapes tests/test_gpu_liquid.py runs, and why.
SHAPES = {
    1: "scalar form; level 65535 (high byte 255: lane 63, walk position 3)",
    2: "scalar form; row sum 2^15",
    3: "scalar form",
    5: "scalar form; lo == hi on the 0.25 and 0.75 ranks",
    261: "histogram tail loops only; lo == hi",
    262: "tail loops only; the one shape where the 0.25 ranks can sit on levels 255 | 256",
    900: "one pass of the four-in-flight histogram loops plus a tail; the 0.75 ranks on 255 | 256",
    2051: "the scalar twin of 2308",
    2308: "vector form; one pass of k_quantise's eight-in-flight loops plus a tail of 260",
    65540: "counts above 65535 in one histogram bin; every level 0 in `flat`",
}
VERSION = {
    "yuma4": "Yuma 4 (Rhef+relative bonds) - liquid alpha on",
    "yuma1": "Yuma 1 (paper) - liquid alpha on",
    "yuma2": "Yuma 2 (Adrian-Fish)",
    "rust": "Yuma 0 (subtensor)",
}
OTHER_VARIANT_SHAPES = (5, 900, 2308)  # Yuma 1, Yuma 2 and YumaRust run on these


def row_sum(M: int) -> int:
    return 1 << (15 if M <= 2 else 17)


def families(M: int) -> tuple[str, ...]:
    """The families a shape admits, in epoch order (`zero` never first)."""
    if M <= 3:
        return ("top", "flat", "zero") if M == 2 else ("top", "zero")
    if M == 5:
        return ("top", "flat", "zero")
    out = ["sparseA"]
    if M <= 25000:
        out.append("sparseB")
    if M <= 1000 and (M - 1) % 4:
        out.append("straddle75")
    if M <= 340 and (M - 1) % 4:
        out.append("straddle25")
    if M <= 25000:
        out.append("spread")
    # the NaN epochs last: a Yuma 4 bond state that has met a NaN alpha stays NaN
    return tuple(out + ["flat", "zero"])


@dataclass(frozen=True)
class Config:
    """What the oracle reads from a configuration (yumas.py:7-26)."""
    kappa: float = 0.5
    consensus_precision: int = 100000
    bond_penalty: float = 0.99
    bond_alpha: float = 0.1
    liquid_alpha: bool = True
    alpha_high: float = 0.9
    alpha_low: float = 0.7
    decay_rate: float = 0.1
    capacity_alpha: float = 0.1
    override_consensus_high: float | None = None
    override_consensus_low: float | None = None


def ranks(M: int, q: float) -> tuple[int, int, float]:
    """(lo, hi, w) of torch.quantile on M values: rank = fp32(q) * (M - 1) in fp32."""
    rank = F32(F32(q) * F32(M - 1))
    lo = int(rank)
    return lo, int(math.ceil(float(rank))), float(F32(rank - F32(lo)))


def levels_of(w: np.ndarray, M: int, as_double: bool = False) -> np.ndarray:
    """The quantisation levels of a weight row every validator gives (yumas.py:211; :97 in fp64)."""
    craw = np.maximum(np.asarray(w, np.int64), 1).astype(np.float64) / row_sum(M)
    q = orc.quantise(craw if as_double else craw.astype(F32), as_double)
    return np.rint(q.astype(np.float64) * 65535.0).astype(np.int64)


def _weights(target: np.ndarray, M: int, n_fill: int) -> np.ndarray:
    """A weight row whose leading columns have the levels `target` (ascending;
    level 0 is weight 0) and whose last n_fill columns share the remainder of
    the row sum, none of them below the largest targeted weight."""
    target = np.asarray(target, np.int64)
    assert len(target) + n_fill == M and n_fill >= 1
    Z = int((target == 0).sum())
    s = Fraction(row_sum(M) + Z, 65535)  # weight per level: sum(C_raw) = (rowsum + Z) / rowsum
    w = np.array([0 if t == 0 else math.ceil((int(t) + Fraction(1, 2)) * s) for t in target], dtype=np.int64)
    rem = row_sum(M) - int(w.sum())
    fill = np.array([rem // n_fill + (1 if i >= n_fill - rem % n_fill else 0) for i in range(n_fill)], dtype=np.int64)
    assert rem >= 0 and fill.min() >= max(int(w.max(initial=0)), 1) and fill.max() <= 65535, (M, rem, n_fill)
    w = np.concatenate([w, fill])
    assert int(w.sum()) == row_sum(M)
    assert (levels_of(w, M)[:len(target)] == target).all()
    return w


def _rising(n: int, M: int, budget_levels: int, first: int = 1) -> np.ndarray:
    """n ascending levels first, first + 1, ... in equal runs, as many distinct
    ones (at most 200) as `budget_levels` (a sum of levels) pays for."""
    if n <= 0:
        return np.zeros(0, np.int64)
    best = np.full(n, first, np.int64)
    for K in range(2, 201):
        lv = first + (np.arange(n, dtype=np.int64) * K) // n
        if int(lv.sum()) + n > budget_levels:
            break
        best = lv
    return best


def _sparse(M: int, straddle: bool) -> np.ndarray:
    n_fill = 2
    lo99, hi99, _ = ranks(M, 0.99)
    Z = max(math.ceil(0.76 * M), ranks(M, 0.75)[1] + 1)
    scale = (row_sum(M) + Z) / 65535.0
    budget = int((row_sum(M)) / scale)  # levels the row sum pays for
    if not straddle:
        # the fillers stay on top: two levels above the 200 that _rising stops at
        mid = _rising(M - Z - n_fill, M, budget - 2 * 202)
        return _weights(np.concatenate([np.zeros(Z, np.int64), mid]), M, n_fill)
    # levels 255 on ranks .. lo99, 256 from hi99 on
    n_top = M - n_fill - hi99
    assert n_top >= 1 and lo99 + 1 == hi99
    run = min(3, lo99 + 1 - Z)
    n = lo99 + 1 - Z - run
    left = budget - 256 * (n_top + n_fill) - 255 * run - 64
    mid = _rising(n, M, left)
    assert mid.size == 0 or mid.max() < 255
    target = np.concatenate([np.zeros(Z, np.int64), mid, np.full(run, 255), np.full(n_top, 256)])
    return _weights(target, M, n_fill)


def _flat(M: int) -> np.ndarray:
    if M == 2:
        return np.array([1 << 14, 1 << 14], dtype=np.int64)
    total = row_sum(M)
    if ranks(M, 0.99)[1] <= M - 2:   # the remainder above: on the top column
        base = total // M
        w = np.full(M, base, np.int64)
        w[-1] = total - base * (M - 1)
    else:                            # below: the 0.25 ranks stay off position 0
        assert ranks(M, 0.25)[0] >= 1
        base = -(-total // M)
        w = np.full(M, base, np.int64)
        w[0] = total - base * (M - 1)
    assert 0 <= w.min() and w.max() <= 65535 and int(w.sum()) == total
    return w


def _straddle(M: int, q: float) -> np.ndarray:
    n_fill = 2
    lo, hi, _ = ranks(M, q)
    assert hi == lo + 1
    n_top = M - n_fill - hi
    budget = 65535 - 258 * n_top - 255 - 2 * 300 - 3 * (M - n_top)
    assert n_top >= 1 and budget > lo, (M, q)
    low = _rising(lo, M, budget)
    # 255 | 256, 257, 258 ...: one step of either rank, either way, is another level
    target = np.concatenate([low, [255], 256 + np.minimum(np.arange(n_top, dtype=np.int64), 2)])
    return _weights(target, M, n_fill)


def _spread(M: int) -> np.ndarray:
    n_fill = 2
    cls = 1 + np.arange(M - n_fill, dtype=np.int64) % 97
    base = 1
    while int(((base + 1) * cls).sum()) + 2 * (base + 1) * 97 <= row_sum(M):
        base += 1
    w = base * cls
    rem = row_sum(M) - int(w.sum())
    fill = np.array([rem // 2, rem - rem // 2], dtype=np.int64)
    assert fill.min() >= w.max() and fill.max() <= 65535
    return np.concatenate([w, fill])


# Every level of a row is another one, so a selected rank moved by one selects another value.
# M = 2: levels 129 and 65405, so far apart that b - a rounds and the two forms of
# the lerp (w = 0.25 takes one, w = 0.75 the other) give different fp32 values
_TOP = {1: [1 << 15], 2: [65, 32703], 3: [3, 65534, 65535], 5: [2, 9300, 9400, 56135, 56235]}


def family_row(M: int, family: str) -> np.ndarray:
    """The weight row (int64 [M]) of a family, columns in ascending order of weight."""
    if family == "zero":
        return np.zeros(M, np.int64)
    if family == "top":
        w = np.array(_TOP[M], dtype=np.int64)
    elif family == "flat":
        w = _flat(M)
    elif family in ("sparseA", "sparseB"):
        w = _sparse(M, family == "sparseB")
    elif family in ("straddle75", "straddle25"):
        w = _straddle(M, 0.75 if family == "straddle75" else 0.25)
    else:
        assert family == "spread"
        w = _spread(M)
    assert w.shape == (M,) and int(w.sum()) == row_sum(M) and w.min() >= 0 and w.max() <= 65535
    return w


@dataclass
class Inputs:
    M: int
    families: tuple[str, ...]
    W: np.ndarray   # [E, V, M] fp32, raw weights
    S: np.ndarray   # [E, V] fp32, raw stakes


@lru_cache(maxsize=None)
def build(M: int) -> Inputs:
    """The inputs of a shape, one family per epoch (cached: treat them as read-only)."""
    fams = families(M)
    assert fams[0] != "zero" and len(fams) <= 7
    rng = np.random.default_rng([0x11901D, M])
    rows = [family_row(M, f)[rng.permutation(M)] for f in fams]
    W = np.broadcast_to(np.stack(rows).astype(F32)[:, None, :], (len(fams), V, M)).copy()
    S = np.full((len(fams), V), STAKE_TOTAL // V, dtype=F32)
    W.setflags(write=False)
    S.setflags(write=False)
    return Inputs(M, fams, W, S)


# ---------------------------------------------------------------------------
# the reference: oracle.run, and the oracle's liquid-alpha block per epoch
# ---------------------------------------------------------------------------
def levels(C: np.ndarray) -> np.ndarray:
    """The integer levels of a quantised consensus C = level / 65535."""
    lv = np.rint(np.asarray(C, np.float64) * 65535.0).astype(np.int64)
    assert ((lv.astype(F32) / F32(65535.0)).astype(F32) == np.asarray(C, F32)).all()
    return lv


def quantile_exact(lv, q: float) -> np.float32:
    """torch.quantile on levels / 65535 in rational arithmetic: sort Python
    ints, then the lerp in Fractions with one rounding to fp32. Where b - a is
    an fp32 value (every case but levels more than a factor of two apart) that
    is round(a + w (b - a)) in either form; elsewhere d = round(b - a) first,
    and the form torch takes for this w: a + w d, or b - d (1 - w)."""
    s = sorted(int(x) for x in lv)
    lo, hi, _ = ranks(len(s), q)
    rank = Fraction(float(F32(F32(q) * F32(len(s) - 1))))
    w = rank - lo
    assert Fraction(float(F32(float(w)))) == w and Fraction(float(F32(float(1 - w)))) == 1 - w  # both exact in fp32
    a, b = (Fraction(float(F32(F32(x) / F32(65535.0)))) for x in (s[lo], s[hi]))
    d = Fraction(float(orc._round_f32(b - a)))
    if d == b - a:
        return orc._round_f32(a + w * (b - a))
    return orc._round_f32(a + w * d if w < Fraction(1, 2) else b - d * (1 - w))


def alpha_unclamped(C: np.ndarray, a, b) -> np.ndarray:
    """1 / (1 + e^(-a C + b)) in fp64, from the fp32 a and b."""
    with np.errstate(over="ignore", invalid="ignore"):
        y = -np.float64(F32(a)) * np.asarray(C, np.float64) + np.float64(F32(b))
        return 1.0 / (1.0 + np.exp(y))


@lru_cache(maxsize=None)
def reference(M: int, variant: str = "yuma4", cfg: Config = Config(), epochs: tuple | None = None) -> dict:
    """oracle.run on build(M) (the epochs `epochs`, default all) and, per
    epoch, oracle.liquid_alpha on the oracle's C: Dn, C, I, B as oracle.run
    gives them, ab [E, 2] (fp32 a, b), bond_alpha [E, M], alpha [E, M] (the
    unclamped alpha in fp64), high / low [E] (the consensus_high / _low the
    fit used). Cached: read-only."""
    inp = build(M)
    idx = list(range(len(inp.families))) if epochs is None else list(epochs)
    out = dict(orc.run(VERSION[variant], inp.W[idx], inp.S[idx], cfg))
    E = len(idx)
    out["ab"] = np.full((E, 2), np.nan, F32)
    out["bond_alpha"] = np.full((E, M), np.nan, F32)
    out["alpha"] = np.full((E, M), np.nan)
    if cfg.liquid_alpha:
        for e in range(E):
            ba, a, b = orc.liquid_alpha(out["C"][e], cfg)
            out["ab"][e] = (F32(a), F32(b))
            out["bond_alpha"][e] = ba
            out["alpha"][e] = alpha_unclamped(out["C"][e], a, b)
    for v in out.values():
        v.setflags(write=False)
    return out


def with_overrides(cfg: Config, high=None, low=None, liquid=True) -> Config:
    return replace(cfg, override_consensus_high=high, override_consensus_low=low, liquid_alpha=liquid)
