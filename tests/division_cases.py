"""Edge rows for the weight normalisation W / (row sum + 1e-6) and the column
division S*W_b / column sum, and a reference that is exact for them.

Host side only (numpy, no GPU, no engine). tests/test_division_cases_host.py
proves the properties claimed here; tests/test_gpu_division_forms.py drives
every kernel form that divides on these inputs and compares every element bit
for bit.

Two observations carry the exact reference.

1. Row sums that do not depend on the summation order. Every row is built from
   "big" entries, integers times ONE power of two whose exact total stays below
   2^24 of that unit (so every partial sum of bigs is exact), and optionally
   "small" entries whose absolute total is below a quarter ulp of the smallest
   nonzero big entry (so a partial sum of smalls never moves a partial sum that
   holds a big, and the smalls among themselves are integers times one power of
   two again, exact). Every order then gives RN(exact sum); rs = RN(sum + 1e-6f)
   is one more rounding and in general no power of two: the quotients are
   inexact and the correction step of the reciprocal division does real work.

2. A Yuma 4 epoch with bond_alpha = 0.5, no liquid alpha and zero bonds is
   B = min(0 + min(0.5 * Wn, 1), 1): the halving is exact (except on a subnormal
   odd quotient, where both sides round alike), so B shows the bits of Wn as
   every element-wise bond kernel forms it, with one exception: 0 + (-0) is +0,
   so B cannot show the sign of a zero quotient. The element-wise bond scans
   are not tested for the -0 family; the sign of a zero Wn is held through the
   materialised Wn alone.

Row families of the tame epoch (epoch 0; `Inputs.rows`), named by the side of
the division guard (|a|, |d| in [2^-60, 2^60] or a == +-0; yuma_engine.hip,
row_div / div_fast / screen_ok) they are on:
  plain     integers 0 .. 999, about 30 % zeros
  lo-in     plain, the smallest nonzero weight exactly 2^-60 (inside: inclusive)
  lo-out    the same row with nextafter(2^-60, 0)
  hi-in     one weight 2^60, the row sum exactly 2^60 (the plain integers beside
            it are far below a quarter ulp of 2^60)
  hi-near   a plain row times a power of two that puts the row sum into
            [2^59, 2^60): the divisor just inside, the quotients inexact (hi-in's
            divisor is a power of two, so its quotients cannot be)
  hi-out    a weight of nextafter(2^60, inf) in an otherwise plain row
  hi-sum    two weights of 2^60: every weight inside, the row sum 2^61 outside
  down      a plain row times 2^-70: every weight below the guard, rs ~ 1e-6
  up        a plain row times 2^50: rs > 2^60
  subnormal integers times 2^-149 beside plain integers
  tiny-q    {k 2^60, 2^-70, 2^-80, 2^-100}: subnormal and zero quotients
  zero      an all-zero row
  mzero     -0.0 entries among plain ones, one of them in the all-zero column
The tame epoch has one all-zero column (zero_column): C is +0 there.
Signed epoch (1): `neg` (a plain row negated: negative rs), `cancel` (+k / -k
pairs: the sum is exactly 0, rs = 1e-6f, quotients around 1e9). Non-finite epoch
(2): one NaN, one +inf, one -inf, each in its own otherwise plain row.

The edge rows sit at row 0, row V - 1 and on both sides of the row-group
boundaries of the kernel forms (4, 16, 64, 256, 1024), every other row is
plain: no wave of any form sees only plain rows, and every tile holds plain
rows beside the edge rows, so a redo of the tile after `slow` has to keep the
fast-path rows' bits too.

Stakes are dyadic and total exactly 1 (subset sums and S * x are exact):
"spread" stakes most rows, ("pair", i, j) gives rows i and j one half each, so a
column sum over validators has at most two nonzero terms: one rounding in any
order."""

from __future__ import annotations

from dataclasses import dataclass
from fractions import Fraction
from functools import lru_cache

import numpy as np

from oracle import yuma_oracle as orc

F32 = np.float32
EPS = F32(1e-6)
LO, HI = F32(2.0 ** -60), F32(2.0 ** 60)
TAME = ("lo-in", "lo-out", "hi-in", "hi-out", "down", "up", "zero", "subnormal", "tiny-q", "mzero", "hi-near",
        "hi-sum")
SIGNED = ("neg", "cancel")
NONFINITE = ("nan", "+inf", "-inf")
INSIDE = ("plain", "lo-in", "hi-in", "hi-near", "zero", "mzero")  # the row passes row_div and screen_ok
BOUNDARIES = (4, 16, 64, 256, 1024)

# (V, M) of the GPU case table (tests/test_gpu_division_forms.py)
SHAPES = ((13, 36), (16, 36), (40, 132), (64, 132), (70, 260), (70, 262), (200, 132), (256, 260), (300, 68), (300, 67),
          (1100, 96), (70, 1024), (70, 16384))


@dataclass
class Inputs:
    V: int
    M: int
    stake: object
    W: np.ndarray        # [3, V, M] fp32: tame, signed, non-finite
    S: np.ndarray        # [3, V] fp32, raw stakes (integers; S / S.sum() is exact)
    W_plain: np.ndarray  # [V, M]: the tame epoch with every edge row replaced by a plain row
    rows: dict           # family -> row indices (tame families, then the signed and non-finite ones)
    edge_rows: tuple     # the positions that hold an edge row in some epoch

    def family_of(self, epoch: int) -> dict:
        names = (TAME, SIGNED, NONFINITE)[epoch]
        fam = {int(r): n for n in names for r in self.rows.get(n, ())}
        return {v: fam.get(v, "plain") for v in range(self.V)}


def edge_positions(V: int) -> list:
    """Row 0, row V - 1, both sides of every row-group boundary inside V, then
    even rows from row 6, until every tame family has a row (V - 5 rows at the
    most: the 13-validator shape holds the first eight families, the
    16-validator shape the last four and the first six)."""
    pos = [0, V - 1]
    for b in BOUNDARIES:
        if b < V - 1:
            pos += [b - 1, b]
    pos += [r for r in range(6, V - 1, 2)] + [5]
    out = []
    for p in pos:
        if p not in out:
            out.append(p)
    n = min(V - 5, max(len(TAME), 2 + 2 * sum(b < V - 1 for b in BOUNDARIES)))
    return out[:n]


def zero_column(M: int) -> int:
    """The all-zero column of the tame and the plain-only epoch: C is +0 there."""
    return M // 2


def _plain(rng, M: int, zc=None, zeros: bool = True) -> np.ndarray:
    w = rng.integers(1, 1000, M).astype(np.float64)
    if zeros:
        w[rng.random(M) < 0.3] = 0.0
        w[_spots(rng, M, 1, zc)] = 999.0   # never all-zero
    if zc is not None:
        w[zc] = 0.0
    return w


def _spots(rng, M: int, n: int, zc=None) -> np.ndarray:
    return rng.choice(np.array([m for m in range(M) if m != zc]), size=n, replace=False)


def _tame_row(rng, name: str, M: int) -> np.ndarray:
    zc = zero_column(M)
    w = _plain(rng, M, zc)
    if name in ("lo-in", "lo-out"):
        w[w == 1.0] = 2.0  # (the smallest nonzero weight is the planted one either way)
        w[_spots(rng, M, 1, zc)] = float(LO) if name == "lo-in" else float(np.nextafter(LO, F32(0)))
    elif name == "hi-in":
        w[_spots(rng, M, 1, zc)] = float(HI)
    elif name == "hi-near":
        total = int(w.sum())
        w *= 2.0 ** (59 - (total.bit_length() - 1))  # the sum lands in [2^59, 2^60)
    elif name == "hi-out":
        w[_spots(rng, M, 1, zc)] = float(np.nextafter(HI, F32(np.inf)))
    elif name == "hi-sum":
        w[_spots(rng, M, 2, zc)] = float(HI)
    elif name == "down":
        w *= 2.0 ** -70
    elif name == "up":
        w *= 2.0 ** 50
    elif name == "subnormal":
        at = _spots(rng, M, min(6, M // 4), zc)
        w[at] = rng.integers(1, 1000, at.size) * 2.0 ** -149
    elif name == "tiny-q":
        w[:] = 0.0
        at = _spots(rng, M, 6, zc)
        w[at] = [2.0 ** 60, 3 * 2.0 ** 60, 5 * 2.0 ** 60, 2.0 ** -70, 2.0 ** -80, 2.0 ** -100]
    elif name == "zero":
        w[:] = 0.0
    elif name == "mzero":
        z = np.nonzero(w == 0.0)[0]
        w[z[::2]] = -0.0
        w[_spots(rng, M, 1, zc)] = -0.0
        w[zc] = -0.0  # a -0 weight under C = +0: the tie of the two zeros in min(Wn, C)
    else:
        raise AssertionError(name)
    return w


def _signed_row(rng, name: str, M: int) -> np.ndarray:
    w = _plain(rng, M)
    if name == "neg":
        return -w
    assert name == "cancel"
    half = M // 2
    w[half:2 * half] = -w[:half]
    w[2 * half:] = 0.0
    return w[rng.permutation(M)] + 0.0  # (no -0 entry: the zeros are +0)


def stakes(V: int, stake, edges) -> np.ndarray:
    """Raw stakes [V], integers: "spread" totals 2^16 units (every edge row is
    staked, every fourth plain row is not); ("pair", i, j) is 1 for i and j."""
    u = np.zeros(V, dtype=np.int64)
    if stake == "spread":
        plain = [v for v in range(V) if v not in edges]
        staked = [v for v in range(V) if v in edges or plain.index(v) % 4 != 1]
        u[staked] = 1 + np.arange(len(staked)) % 3
        u *= (1 << 16) // int(u.sum())
        first_plain = next(v for v in staked if v not in edges)
        u[first_plain] += (1 << 16) - int(u.sum())
        assert int(u.sum()) == 1 << 16
    else:
        kind, i, j = stake
        assert kind == "pair" and i != j
        u[[i, j]] = 1
    return u.astype(F32)


@lru_cache(maxsize=None)
def build(V: int, M: int, stake="spread") -> Inputs:
    """The inputs for a V x M subnet (cached: treat them as read-only)."""
    rng = np.random.default_rng([0xD171DE, V, M])
    pos = edge_positions(V)
    # tame: an all-zero column; non-finite: no zero weight (every C is positive, so the -0
    # quotients of the -inf row meet no +0 in min(Wn, C))
    W = np.stack([np.stack([_plain(rng, M, zero_column(M) if e == 0 else None, e != 2) for _ in range(V)])
                  for e in range(3)])
    W_plain = W[0].copy()
    rows: dict = {}
    tame = TAME[8:] + TAME[:8] if V == 16 else TAME  # 16 validators: the families the 13-validator shape lacks
    for k, r in enumerate(pos):
        for e, names in enumerate((tame, SIGNED)):
            name = names[k % len(names)]
            W[e, r] = (_tame_row, _signed_row)[e](rng, name, M)
            rows.setdefault(name, []).append(r)
    for k, name in enumerate(NONFINITE):
        r = pos[k]
        W[2, r, rng.integers(0, M)] = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}[name]
        rows[name] = [r]
    rows["plain"] = [v for v in range(V) if v not in pos]
    W32 = W.astype(F32)
    assert np.array_equal(W32.astype(np.float64), W, equal_nan=True)  # every planted value is an fp32
    S = np.broadcast_to(stakes(V, stake, set(pos)), (3, V)).copy()
    Wp = W_plain.astype(F32)
    for a in (W32, S, Wp):
        a.setflags(write=False)
    return Inputs(V, M, stake, W32, S, Wp, rows, tuple(pos))


# ---------------------------------------------------------------------------
# exact sums, the guard restated, the reference
# ---------------------------------------------------------------------------
def exact_sum(row) -> Fraction:
    """The exact sum of a finite fp32 row."""
    m, e = np.frexp(np.asarray(row, np.float64))
    mi = (m * 2.0 ** 53).astype(np.int64)
    nz = mi != 0
    if not nz.any():
        return Fraction(0)
    emin = int(e[nz].min())
    total = sum(int(a) << (int(b) - emin) for a, b in zip(mi[nz].tolist(), e[nz].tolist()))
    return Fraction(total) * Fraction(2) ** (emin - 53)


def row_sums(W) -> np.ndarray:
    """rs = fp32 row sum + 1e-6f (yumas.py:186), numpy's order."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(W, F32).sum(axis=-1, dtype=F32) + EPS).astype(F32)


def normalise(W) -> np.ndarray:
    """IEEE fp32 W / rs."""
    W = np.asarray(W, F32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        return (W / row_sums(W)[..., None]).astype(F32)


def in_guard(x) -> np.ndarray:
    """|x| in [2^-60, 2^60] (false for NaN and inf)."""
    a = np.abs(np.asarray(x, F32))
    with np.errstate(invalid="ignore"):
        return (a >= LO) & (a <= HI)


def row_div_ok(rs) -> np.ndarray:
    """row_div's `ok`: the divisor is inside the guard."""
    return in_guard(rs)


def screen_ok(W) -> np.ndarray:
    """screen_ok on the rows of W [.., M], as k_rowsum forms it: the largest |w|
    and the smallest nonzero |w|, as bit patterns, against 2^60 and 2^-60 (a zero
    wraps to the top of `bmin1` and never lowers it)."""
    b = (np.asarray(W, F32).view(np.uint32) & np.uint32(0x7FFFFFFF)).astype(np.int64)
    bmax = b.max(axis=-1)
    bmin1 = ((b - 1) & 0xFFFFFFFF).min(axis=-1)
    lo, hi = int(LO.view(np.uint32)), int(HI.view(np.uint32))
    return (bmax <= hi) & ((bmin1 == 0xFFFFFFFF) | (bmin1 + 1 >= lo))


def fast_row(W) -> np.ndarray:
    """Rows whose every quotient takes the fast path: fast_row_rcp is no NaN."""
    return row_div_ok(row_sums(W)) & screen_ok(W)


def slow_elements(W) -> np.ndarray:
    """div_fast's `slow` per element."""
    W = np.asarray(W, F32)
    return ~(row_div_ok(row_sums(W))[..., None] & (in_guard(W) | (W == 0)))


@dataclass(frozen=True)
class Params:
    """What oracle.epoch reads of a YumaConfig."""
    kappa: float = 0.5
    consensus_precision: int = 100000
    bond_alpha: float = 0.5
    bond_penalty: float = 0.0
    liquid_alpha: bool = False
    capacity_alpha: float = 0.1
    decay_rate: float = 0.1
    alpha_high: float = 0.9
    alpha_low: float = 0.7
    override_consensus_high: object = None
    override_consensus_low: object = None


def yuma4_bits(Wn, alpha=0.5, B_old=None) -> np.ndarray:
    """Observation 2 in plain numpy: one Yuma 4 epoch on normalised weights."""
    a = F32(alpha)
    Wn = np.asarray(Wn, F32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        if B_old is None:
            return np.minimum((F32(0.0) + np.minimum((a * Wn).astype(F32), F32(1.0))).astype(F32), F32(1.0))
        Bd = (np.asarray(B_old, F32) * F32(1 - alpha)).astype(F32)
        rem = np.maximum((F32(1.0) - Bd).astype(F32), F32(0.0))
        return np.minimum((Bd + np.minimum((a * Wn).astype(F32), rem)).astype(F32), F32(1.0))


def epochs_of(inp: Inputs, order) -> tuple:
    """W [E, V, M], S [E, V] of an epoch order: 0 / 1 / 2, or "plain"."""
    W = np.stack([inp.W_plain if e == "plain" else inp.W[e] for e in order])
    return W, np.stack([inp.S[0]] * len(order))


_REF: dict = {}


def reference(V: int, M: int, stake="spread", order=(0,), version="Yuma 4 (Rhef+relative bonds)", **cfg) -> dict:
    """oracle.run over the epoch order (cached, read-only): Wn, C, I, Dn, B [E, ...],
    Wc, R per epoch from oracle.epoch, and `fast` [E, V], the expected side of the
    row screen."""
    key = (V, M, stake, tuple(order), version, tuple(sorted(cfg.items())))
    if key not in _REF:
        inp = build(V, M, stake)
        W, S = epochs_of(inp, order)
        p = Params(**cfg)
        with np.errstate(all="ignore"):
            out = orc.run(version, W, S, p, return_weight=True)
            variant = orc.VERSIONS[version][0]
            first = orc.epoch(variant, W[0], S[0], None, p)
        out["Wc"] = first["consensus_clipped_weight"]
        out["R"] = first["server_rank"]
        out["P"] = first["server_prerank"]
        for k in ("weight_for_bond", "validator_bond"):
            if k in first:
                out[k] = first[k]
        out["fast"] = np.stack([fast_row(w) for w in W])
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = out
    return _REF[key]


# ---------------------------------------------------------------------------
# the case table of tests/test_gpu_division_forms.py (data only; the host test
# holds it to engine.scan_plan and to the validator ranges of DESIGN.md 2.0)
# ---------------------------------------------------------------------------
Y0, Y1, Y2, Y3, Y4 = range(5)
VERSION = {Y0: "Yuma 0 (subtensor)", Y1: "Yuma 1 (paper)", Y2: "Yuma 2 (Adrian-Fish)", Y3: "Yuma 3 (Rhef)",
           Y4: "Yuma 4 (Rhef+relative bonds)"}


@dataclass(frozen=True)
class Case:
    id: str
    kind: str            # wn | wn2 | bonds | grp | col | y3pair
    V: int
    M: int
    rank: str            # the phase-1 rank kernel the shape is meant to reach
    scan: tuple          # (form, shape, rq) of the bond scan
    variant: int = Y4
    want: tuple = ()
    hist: bool = False
    opts: tuple = ()     # run() keywords as (name, value) pairs

    @property
    def kw(self):
        return dict(self.opts)


TILE, WIDE_, FLAT, FLAT_S = ("k_bonds_elem", "tile_hist", False), ("k_bonds_elem", "wide", False), \
    ("k_bonds_elem", "flat1", True), ("k_bonds_elem", "flat1", False)
GRP = ("k_bonds_grp", None, True)
FULL = {13: "k_rank_w<1", 16: "k_rank_w<1", 40: "k_rank_w<4", 64: "k_rank_w<4", 70: "k_rank_w<16", 200: "k_rank_w<16",
        256: "k_rank_w<16", 300: "k_rank<1024, 16>", 1100: "k_rank_sw<BIGV> + k_full_big"}


def _cases():
    out = []
    for V, M in SHAPES:  # 1. materialised Wn / Wc (Yuma 3)
        out.append(Case(f"wn-{V}x{M}", "wn", V, M, FULL[V], FLAT if M % 4 == 0 else FLAT_S, Y3, ("Wn", "Wc", "R")))
    for V, M in ((13, 36), (16, 36), (40, 132), (64, 132), (70, 260), (70, 262)):  # prerank: the k_consensus_w shapes
        out.append(Case(f"wn-P-{V}x{M}", "wn", V, M, FULL[V], FLAT if M % 4 == 0 else FLAT_S, Y3, ("Wn", "Wc", "P")))
    for V, M in ((40, 132), (70, 260), (300, 68), (300, 67), (1100, 96)):  # Yuma 2: the previous slice's div_rn
        scan = ("k_bonds", None, False) if V <= 64 or M % 4 else ("k_bonds_cn", None, True)
        out.append(Case(f"wn2-{V}x{M}", "wn2", V, M, FULL[V], FLAT if V > 1024 else scan, Y2, ("Wn", "Wc")))
    # 2. Wn as the bond kernels form it (Yuma 4, bond_alpha 0.5)
    rank = lambda V, M: "k_rank_sw<BIGV>" if V > 1024 else "k_rank_sw" if M >= 16384 else "k_rank_s"
    for V, M in SHAPES:
        if M % 4:
            out.append(Case(f"elem-scalar-hist-{V}x{M}", "bonds", V, M, rank(V, M), FLAT_S, hist=True))
            out.append(Case(f"elem-scalar-{V}x{M}", "bonds", V, M, rank(V, M), FLAT_S))
        else:
            out.append(Case(f"elem-hist-{V}x{M}", "bonds", V, M, rank(V, M), WIDE_ if M >= 1024 else TILE, hist=True))
    for V, M in ((13, 36), (70, 260), (300, 68), (1100, 96), (70, 16384)):
        out.append(Case(f"elem-flat-{V}x{M}", "bonds", V, M, rank(V, M), FLAT, want=("R",)))
    V, M = 70, 260
    for name, scan, hist, opts in (
            ("SC", TILE, True, (("sched", "identity"),)), ("SC-flat", FLAT, False, (("sched", "identity"),)),
            ("MV", FLAT, False, (("want_move", True),)), ("RS", FLAT, False, (("want_row_stats", True),)),
            ("RL", FLAT, False, (("resets", ()),)), ("RL-hist", TILE, True, (("resets", ()),)),
            ("RW", FLAT, False, (("row_resets", ()),)), ("RW-hist", TILE, True, (("row_resets", ()),)),
            ("strided", TILE, True, (("hist_stride", 2), ("hist_first", 0))),
            ("bf16", TILE, True, (("hist_dtype", "bfloat16"),)),
            ("watch", FLAT, False, (("watch", "spread"),)), ("rows", FLAT, False, (("watch_rows", "edges"),))):
        out.append(Case(f"elem-{name}-{V}x{M}", "bonds", V, M, "k_rank_s", scan, hist=hist, opts=opts))
    out.append(Case("elem-bf16-70x1024", "bonds", 70, 1024, "k_rank_s", WIDE_, hist=True, opts=(("hist_dtype", "bfloat16"),)))
    out.append(Case("elem-strided-70x1024", "bonds", 70, 1024, "k_rank_s", WIDE_, hist=True,
                    opts=(("hist_stride", 2), ("hist_first", 0))))
    for V, M in ((13, 36), (70, 260), (300, 68)):  # the shared-input sweep, N = 4
        out.append(Case(f"grp-hist-{V}x{M}", "grp", V, M, "k_rank_mc" if V <= 256 else "k_rank_s", GRP, hist=True))
        out.append(Case(f"grp-{V}x{M}", "grp", V, M, "k_rank_mc" if V <= 256 else "k_rank_s", GRP))
    out.append(Case("y3-pair-70x260", "y3pair", 70, 260, "k_rank_s", TILE, Y3, hist=True))
    out.append(Case("y3-pair-flat-70x260", "y3pair", 70, 260, "k_rank_s", FLAT, Y3))
    # 3. the column division under pair stakes
    kb, cn = ("k_bonds", None, False), ("k_bonds_cn", None, True)
    for variant in (Y0, Y1, Y2):
        for V, M in ((13, 36), (16, 36), (40, 132)):
            out.append(Case(f"col-y{variant}-{V}x{M}", "col", V, M, "k_rank_s", kb, variant, hist=True))
    for V, M in ((70, 260), (200, 132), (300, 68)):
        out.append(Case(f"col-cn-y0-{V}x{M}", "col", V, M, "k_rank_s", cn, Y0, hist=True))
        out.append(Case(f"col-cn-y1-Wn-{V}x{M}", "col", V, M, FULL[V], cn, Y1, ("Wn",), hist=True))
    for variant in (Y1, Y2):
        out.append(Case(f"col-csb-y{variant}-70x260", "col", 70, 260, "k_rank_sw", TILE, variant, hist=True))
        out.append(Case(f"col-csb-flat-y{variant}-70x260", "col", 70, 260, "k_rank_sw", FLAT, variant))
        out.append(Case(f"col-csb-y{variant}-1100x96", "col", 1100, 96, "k_rank_sw<BIGV>", TILE, variant, hist=True))
    out.append(Case("col-csb-wide-y1-70x1024", "col", 70, 1024, "k_rank_sw", ("k_bonds_elem", "wide", True), Y1, hist=True))
    out.append(Case("col-full-y1-70x260", "col", 70, 260, "k_rank_s", kb, Y1, ("Wb", "B_inst"), hist=True))
    out.append(Case("col-full-y0-scalar-70x262", "col", 70, 262, "k_rank_s", kb, Y0, hist=True))
    out.append(Case("col-big-y0-1100x96", "col", 1100, 96, "k_rank_sw<BIGV>", ("k_rust_big", None, False), Y0, hist=True))
    out.append(Case("col-big-y0-nohist-1100x96", "col", 1100, 96, "k_rank_sw<BIGV>", ("k_rust_big", None, False), Y0))
    return tuple(out)


CASES = _cases()


def rank_kernel(case: Case) -> str:
    """The rank rows of DESIGN.md 2.0 (launch_rank), restated. full: one of Wn /
    Wc / T_v requested; csb: Yuma 1 / 2 above 1024 validators, or above 64 with
    none of Wn / Wc / T_v / W_b / B_inst requested; sweep: shared inputs, N > 1,
    no prerank requested."""
    V, M, want = case.V, case.M, set(case.want)
    if want & {"Wn", "Wc", "Tv"}:
        return FULL[V] if V <= 1024 else "k_rank_sw<BIGV> + k_full_big"
    if V > 1024:
        return "k_rank_sw<BIGV>"
    csb = case.variant in (Y1, Y2) and V > 64 and not want & {"Wb", "B_inst"}
    if csb or M >= 16384:
        return "k_rank_sw"
    if case.kind == "grp" and case.variant != Y2 and V <= 256:
        return "k_rank_mc"
    return "k_rank_s"


def csr_ok(num) -> np.ndarray:
    """The rank pass's column screen, restated for S * W_b [V, M]: csr[m] is
    RN(1 / csb) when the column sum and every nonzero |S W_b| of the column are
    in [2^-60, 2^60], else NaN."""
    num = np.asarray(num, F32)
    csb = num.sum(axis=0, dtype=F32)
    return in_guard(csb) & (in_guard(num) | (num == 0)).all(axis=0)


def tie_rows(case: Case, stake="spread") -> tuple:
    """Rows where min(Wn, C) meets Wn = -0 under C = +0 in the case's run on the
    tame epoch (from the reference): the one place where the result depends on
    which of two equal zeros a minimum returns."""
    order = (0, "plain") if case.kind == "wn2" else (0,)
    ref = reference(case.V, case.M, stake, order, VERSION[case.variant])
    Wn = ref["Wn"][0]
    czero = (ref["C"] == 0).any(axis=0)
    tie = np.signbit(Wn) & (Wn == 0) & czero[None, :]
    return tuple(int(v) for v in np.nonzero(tie.any(axis=1))[0])


def pairs(V: int, M: int) -> list:
    """One (family, edge row, plain row) stake pair per tame family of the shape."""
    inp = build(V, M)
    plain = inp.rows["plain"]
    return [(n, inp.rows[n][0], plain[(k * 7) % len(plain)]) for k, n in enumerate(TAME) if n in inp.rows]
