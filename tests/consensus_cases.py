"""Adversarial inputs for the consensus search, and an exact reference.

Host side only (numpy, no GPU, no engine). Used by
tests/test_consensus_cases_host.py, which proves the properties claimed here,
and by tests/test_gpu_consensus_forms.py, which runs every kernel form of the
consensus pass on them.

Inputs (`build`) are order-independent by construction, so a correct
implementation has to reproduce C bit for bit, on every column:

  * stakes: raw S is integer-valued and totals 2^24 ("u24") or 2^20 ("u20"),
    so S / S.sum() is exact and every subset sum of stakes is exact in fp32;
    "single" gives one validator the whole stake. Some validators hold none.
  * weights: integers <= 65535 (they fit the uint16 input), every row sums to
    a power of two (2^17 in the family epochs), every partial sum is an
    integer below 2^24: rowsum + 1e-6 == rowsum in fp32 and Wn = W / 2^17
    exactly, on the grid of the default precision (17 bisection steps),
    off the 10-step grid of consensus_precision=1000 and on the 24-step grid
    of 10000000. Each row's remainder goes to three filler columns of its
    stake group; no group holds more than fp32(0.3) of the stake, so every
    filler column lands on the lowest grid point and sum(C_raw) stays small.

Epochs: 0 the column families below; 1 every validator's whole row on one
column (Wn == 1.0 exactly, every other column all-zero); 2 (`nonfinite=True`)
the families under another placement with NaN, +inf, -inf, a negative value
and -0.0 in single entries; 3 the families again with one column above 1.0 in
every row (each row's first filler goes negative to pay for it, the row sum
stays 2^17). Only C is compared for epochs 2 and 3.

Column families (names of `Inputs.columns`), all around the grid point T:
  a3 a5 a7      stake above T is exactly floor(fp32(kappa) 2^24) units (for
                "u20" the nearest multiple of 16 below it: 0.3 and 0.7 have no
                exact tie on that stake grid); `+` / `-`: one stake unit more /
                less, by a validator one grid point above T / exactly on T
  b             values T + 128, T, T - 128: the deciding validator sits on a
                grid point of all three precisions
  cmax cmin     the column maximum / minimum is held by a zero-stake validator
  d             the validators with a non-zero weight hold less than every
                kappa: the lowest grid point
  e0 e1 esame   all-zero; one non-zero entry; every validator the same value
  fnarrow fwide bracket widths <= 8 and >= 64 in one lane quad
A full set is placed across the first wave boundary of tile 0; as many
families as fit go to the last, partly filled 64-miner tile (which families
rotates with V + M), and wide shapes get a third set across a tile boundary.
"""

from __future__ import annotations

from dataclasses import dataclass, field
from fractions import Fraction
from functools import lru_cache

import numpy as np

from oracle import yuma_oracle as orc

F32 = np.float32
ROW = 1 << 17        # row sum of the family epochs
T = 512              # the grid point (2^-17 units) the families sit around
ONE_ROW = 1 << 15    # the whole row of the Wn == 1.0 epoch (w >= 32: w / (w + 1e-6) == 1.0f)
KAPPAS = (0.3, 0.5, 0.7)
PRECISIONS = (1000, 100000, 10000000)
NAMES = ("fnarrow", "fwide", "a3", "a3+", "a3-", "a5", "a5+", "a5-", "a7", "a7+", "a7-",
         "b", "cmax", "cmin", "d", "e0", "e1", "esame")
FAMILY = {n: n[0] for n in NAMES}  # a .. f
N_FILL = 3  # filler columns per stake group (a remainder <= 2^17 in three parts fits uint16)


def kappa_units(kappa) -> int:
    """floor(fp32(kappa) * 2^24)."""
    fr = Fraction(float(F32(kappa))) * (1 << 24)
    return fr.numerator // fr.denominator


@dataclass
class Inputs:
    V: int
    M: int
    stake: str
    W: np.ndarray            # [E, V, M] fp32, raw weights
    S: np.ndarray            # [E, V] fp32, raw stakes
    unit: int                # one raw stake unit in units of 2^-24
    roles: dict              # name -> row indices
    columns: dict            # epoch 0: family member name -> columns
    fillers: list
    one_col: int             # the Wn == 1.0 column of epoch 1
    nonfinite: dict = field(default_factory=dict)  # name -> (row, col) of epoch 2; "over": (0, col) of epoch 3

    @property
    def targeted(self):
        return sorted(c for cols in self.columns.values() for c in cols)

    @property
    def last_tile(self) -> range:
        return range(64 * ((self.M - 1) // 64), self.M)


def _split(rng, total: int, n: int, unit: int) -> np.ndarray:
    """n positive multiples of `unit` summing to `total`."""
    k = total // unit
    assert k * unit == total and k >= n
    return (rng.multinomial(k - n, np.full(n, 1.0 / n)) + 1).astype(np.int64) * unit


def _roles(rng, V: int):
    n_zero = max(2, V // 8)
    sizes = [1, 1, 1, 1, 1]  # G3rest, H5, H7, R1rest, R2
    assert V - n_zero - 2 >= 5, "at least 13 validators"
    for i in range(V - n_zero - 2 - 5):
        sizes[i % 5] += 1
    perm = rng.permutation(V)
    out, at = {}, 0
    for name, n in (("Z", n_zero), ("u1", 1), ("u2", 1), ("G3rest", sizes[0]), ("H5", sizes[1]),
                    ("H7", sizes[2]), ("R1rest", sizes[3]), ("R2", sizes[4])):
        out[name] = np.sort(perm[at:at + n])
        at += n
    out["G3"] = np.concatenate([out["u1"], out["G3rest"]])
    out["G5"] = np.concatenate([out["G3"], out["H5"]])
    out["G7"] = np.concatenate([out["G5"], out["H7"]])
    out["R1"] = np.concatenate([out["u2"], out["R1rest"]])
    return out


def _stake_units(rng, roles, V: int, stake: str):
    """Stakes in units of 2^-24, totalling 2^24, and the raw unit."""
    u = np.zeros(V, dtype=np.int64)
    if stake == "single":
        u[roles["H5"][0]] = 1 << 24
        return u, 1
    unit = {"u24": 1, "u20": 16}[stake]
    K3, K5, K7 = ((kappa_units(k) // unit) * unit for k in KAPPAS)
    rest = (1 << 24) - K7
    r1 = (rest // unit // 2) * unit
    u[roles["u1"]] = unit
    u[roles["u2"]] = unit
    u[roles["G3rest"]] = _split(rng, K3 - unit, len(roles["G3rest"]), unit)
    u[roles["H5"]] = _split(rng, K5 - K3, len(roles["H5"]), unit)
    u[roles["H7"]] = _split(rng, K7 - K5, len(roles["H7"]), unit)
    u[roles["R1rest"]] = _split(rng, r1 - unit, len(roles["R1rest"]), unit)
    u[roles["R2"]] = _split(rng, rest - r1, len(roles["R2"]), unit)
    assert int(u.sum()) == 1 << 24
    return u, unit


def _column(rng, name: str, roles, V: int) -> np.ndarray:
    w = np.zeros(V, dtype=np.int64)
    if name[0] == "a":
        A = set(roles["G" + name[1]].tolist())
        w[:] = rng.integers(T - 200, T, V)          # below T
        for v in A:
            w[v] = rng.integers(T + 2, T + 200)
        w[roles["R2"][0]] = T                       # staked, exactly on T: F(T - 1) > F(T)
        w[roles["Z"][0]] = T - 1                    # one grid point below, no stake
        if name.endswith("+"):
            w[roles["u2"]] = T + 1
        if name.endswith("-"):
            w[roles["u1"]] = T
    elif name == "b":
        w[:] = T - 128
        w[roles["H5"]] = T
        w[roles["H7"]] = T
        w[roles["G3"]] = T + 128
    elif name == "cmax":
        w[:] = rng.integers(T - 200, T + 200, V)
        w[roles["Z"][0]] = 20000
    elif name == "cmin":
        w[:] = rng.integers(T - 100, T + 100, V)
        w[roles["Z"][1]] = 0
    elif name == "d":
        w[roles["G3rest"]] = rng.integers(T, T + 100, len(roles["G3rest"]))
    elif name == "e1":
        w[roles["H5"][0]] = T
    elif name == "esame":
        w[:] = T
    elif name == "fnarrow":
        w[:] = rng.integers(1, 7, V)
    elif name == "fwide":
        w[:] = rng.integers(T - 200, T + 200, V)
    else:
        assert name == "e0"
    return w


def _place(names, start: int, room: int):
    """Columns start .. start + room - 1 for as many of `names` as fit, in
    order ("fnarrow" stands for the pair); the (fnarrow, fwide) pair stays
    inside one aligned quad of columns."""
    out, pos, end = [], start, start + room
    queue = [n for n in names if n != "fwide"]
    while queue and pos < end:
        n = queue.pop(0)
        if n != "fnarrow":
            out.append((n, pos))
            pos += 1
        elif pos % 4 == 3 and queue:
            queue.insert(1, n)  # a single first, the pair from the next quad
        elif pos % 4 != 3 and pos + 2 <= end:
            out += [("fnarrow", pos), ("fwide", pos + 1)]
            pos += 2
    return out


def _layout(M: int, rot: int):
    """(family columns, filler columns). rot: which families reach the last tile."""
    assert M >= 36
    rotated = [n for n in NAMES if n not in ("fnarrow", "fwide")]
    r = rot % len(rotated)
    rotated = rotated[r:] + rotated[:r]
    rotated.insert(rot % 3, "fnarrow")
    last0 = 64 * ((M - 1) // 64)
    n_fill = 5 * N_FILL
    if M <= 64:
        placed = _place(NAMES, 0, len(NAMES))
        fillers = list(range(len(NAMES), len(NAMES) + n_fill))
    else:
        placed = _place(NAMES, 8, len(NAMES))                 # across the wave boundary at 16
        fillers = list(range(32, 32 + n_fill))                # 26 .. 31 stay background: a narrow quad in that wave
        placed += _place(rotated, last0, min(M - last0, len(NAMES)))
        if last0 >= 192:
            placed += _place(rotated[5:] + rotated[:5], 120, len(NAMES))  # across the tile boundary at 128
    cols = [c for _, c in placed]
    assert len(set(cols)) == len(cols) and not set(cols) & set(fillers) and max(cols + fillers) < M
    return placed, fillers


def _family_epoch(rng, roles, V: int, M: int, rot: int):
    placed, fillers = _layout(M, rot)
    W = np.zeros((V, M), dtype=np.int64)
    taken = {c for _, c in placed} | set(fillers)
    for j in range(M):  # background: 16-column blocks of narrow (<= 8 grid points) and wider brackets
        if j not in taken:
            W[:, j] = rng.integers(0, 7 if (j // 16) % 2 else 81, V)
    for name, c in placed:
        W[:, c] = _column(rng, name, roles, V)
    groups = [roles["G3"], roles["H5"], roles["H7"], roles["R1"], np.concatenate([roles["R2"], roles["Z"]])]
    row_fill = {}
    for g, rows in enumerate(groups):
        fc = fillers[N_FILL * g:N_FILL * (g + 1)]
        for v in rows:
            rem = ROW - int(W[v].sum())
            assert rem >= N_FILL, "a row overran its budget"
            part = [rem // N_FILL] * N_FILL
            part[0] += rem - sum(part)
            W[v, fc] = part
            row_fill[int(v)] = fc[0]
    assert (W.sum(axis=1) == ROW).all() and W.max() <= 65535 and W.min() >= 0
    return W, placed, fillers, row_fill


@lru_cache(maxsize=None)
def build(V: int, M: int, stake: str = "u24", nonfinite: bool = True) -> Inputs:
    """The inputs for a V x M subnet (cached: treat them as read-only)."""
    rot = V + M
    rng = np.random.default_rng([0xC0115E, V, M, {"u24": 0, "u20": 1, "single": 2}[stake]])
    roles = _roles(rng, V)
    units, unit = _stake_units(rng, roles, V, stake)
    W0, placed, fillers, _ = _family_epoch(rng, roles, V, M, rot)
    columns = {}
    for name, c in placed:
        columns.setdefault(name, []).append(c)
    # epoch 1: the whole row on one column; in the last tile, inside a quad of all-zero columns
    one_col = M - 2
    W1 = np.zeros((V, M), dtype=np.int64)
    W1[:, one_col] = ONE_ROW
    Ws = [W0.astype(F32), W1.astype(F32)]
    nf = {}
    if nonfinite:
        W2i, placed2, _, row_fill = _family_epoch(rng, roles, V, M, rot + 7)
        first = {}
        for name, c in placed2:
            first.setdefault(name, c)
        neg_row, neg_col = int(roles["G3rest"][0]), first["b"]
        # the negative entry: its filler takes the difference, the row still sums to 2^17
        W2i[neg_row, row_fill[neg_row]] += W2i[neg_row, neg_col] + 5
        W2i[neg_row, neg_col] = -5
        zero_row, zero_col = int(roles["R1rest"][0]), first["e0"]
        assert (W2i.sum(axis=1) == ROW).all() and W2i[zero_row, zero_col] == 0
        W2 = W2i.astype(F32)
        W2[zero_row, zero_col] = F32(-0.0)
        nf = {"nan": (int(roles["H5"][0]), first["fwide"]), "+inf": (int(roles["H7"][0]), first["a5"]),
              "-inf": (int(roles["R2"][0]), first["cmin"]), "negative": (neg_row, neg_col),
              "-0.0": (zero_row, zero_col)}
        W2[nf["nan"]] = np.nan
        W2[nf["+inf"]] = np.inf
        W2[nf["-inf"]] = -np.inf
        Ws.append(W2)
        # epoch 3: the families once more, and a column above 1.0 in every row
        # (Wn = 1 + 2^-14): each row's first filler pays for it and goes negative
        W3, placed3, _, row_fill = _family_epoch(rng, roles, V, M, rot + 3)
        over_col = fillers[-1] + 1
        assert over_col not in [c for _, c in placed3] and over_col < M
        for v in range(V):
            W3[v, row_fill[v]] -= ROW + 8 - W3[v, over_col]
            W3[v, over_col] = ROW + 8
        assert (W3.sum(axis=1) == ROW).all() and np.abs(W3).sum(axis=1).max() < 1 << 24
        nf["over"] = (0, over_col)
        Ws.append(W3.astype(F32))
    W = np.stack(Ws)
    S = np.broadcast_to((units // unit).astype(F32), (len(Ws), V)).copy()
    W.setflags(write=False)
    S.setflags(write=False)
    return Inputs(V, M, stake, W, S, unit, roles, columns, fillers, one_col, nf)


# ---------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------
def normalise(W: np.ndarray) -> np.ndarray:
    """fp32 W / (rowsum + 1e-6) (yumas.py:186-187); exact for build()'s finite rows."""
    W = np.asarray(W, F32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        rs = W.sum(axis=-1, dtype=F32)
        return (W / (rs + F32(1e-6))[..., None]).astype(F32)


def normalise_stake(S: np.ndarray) -> np.ndarray:
    S = np.asarray(S, F32)
    return (S / S.sum(dtype=F32)).astype(F32)


def stake_units(Sn: np.ndarray) -> list[int]:
    """Normalised stakes as Python ints in units of 2^-24; asserts that they
    are exact multiples and total <= 1."""
    out = []
    for s in np.asarray(Sn, F32).tolist():
        fr = Fraction(s) * (1 << 24)
        assert fr.denominator == 1 and fr >= 0, f"stake {s} is no multiple of 2^-24"
        out.append(fr.numerator)
    assert sum(out) <= 1 << 24
    return out


def bisect_exact(Wn: np.ndarray, Sn: np.ndarray, kappa: float, precision, trace: list | None = None) -> list[int]:
    """k* per column, C_raw = k* / 2^iters: the reference's bisection
    (yumas.py:195-209) with the stake above the midpoint summed in integers.
    Per step and column: k = (lo + hi) / 2 on the integer grid, the fp32
    midpoint fp32(k / 2^iters), `Wn > mid` in fp32, the stake above it as an
    exact integer number of 2^-24 units, compared with fp32(kappa) as a
    rational. trace: appended per step with a dict of per-column lists
    k, units (the exact stake above) and on_grid (a staked validator's Wn
    equals the midpoint)."""
    Wn = np.asarray(Wn, F32)
    V, M = Wn.shape
    iters = orc.bisect_iterations(precision)
    top = 1 << iters
    units = stake_units(Sn)
    u64 = np.array(units, dtype=np.int64)
    staked = u64 > 0
    kap = Fraction(float(F32(kappa)))
    kap_num, kap_den = kap.numerator << 24, kap.denominator  # units / 2^24 > kappa <=> units * den > num
    lo, hi = [0] * M, [top] * M
    for _ in range(iters):
        k = [(a + b) // 2 for a, b in zip(lo, hi)]
        assert all(2 * x == a + b for x, a, b in zip(k, lo, hi))  # the double midpoint is this grid point
        mid = np.array([F32(x / top) for x in k], dtype=F32)
        assert (mid.astype(np.float64) * top == np.array(k, dtype=np.float64)).all()  # fp32(k / 2^iters) is exact
        above = Wn > mid[None, :]
        exact = [int(x) for x in (above.T.astype(np.int64) @ u64)]
        if trace is not None:
            on = ((Wn == mid[None, :]) & staked[:, None]).any(axis=0)
            trace.append({"k": k, "units": exact, "on_grid": on.tolist()})
        for m in range(M):
            if exact[m] * kap_den > kap_num:
                lo[m] = k[m]
            else:
                hi[m] = k[m]
    return hi


def consensus_exact(Wn, Sn, kappa, precision, as_double: bool = False) -> np.ndarray:
    """The quantised consensus C [M] from bisect_exact and oracle.quantise."""
    top = 1 << orc.bisect_iterations(precision)
    raw = np.array([k / top for k in bisect_exact(Wn, Sn, kappa, precision)], dtype=np.float64)
    return orc.quantise(raw if as_double else raw.astype(F32), as_double)


@lru_cache(maxsize=None)
def reference_C(V: int, M: int, stake: str, kappa: float, precision, as_double: bool = False) -> np.ndarray:
    """consensus_exact for every epoch of build(V, M, stake): C [E, M] (cached, read-only)."""
    inp = build(V, M, stake)
    out = np.stack([consensus_exact(normalise(inp.W[e]), normalise_stake(inp.S[e]), kappa, precision, as_double)
                    for e in range(inp.W.shape[0])])
    out.setflags(write=False)
    return out


def bracket(Wn: np.ndarray, Sn: np.ndarray, kappa: float, iters: int):
    """The search's starting bracket (lo, hi) per column, as the kernels and
    tests/test_consensus_hist.py::hist_consensus form it from the real rows."""
    top = 1 << iters
    scale = F32(top)
    bits = np.asarray(Wn, F32).view(np.int32)
    imax, imin = bits.max(axis=0), bits.min(axis=0)
    nanc = imax > 0x7F800000
    vmax = imax.astype(np.int32).view(F32)
    vmin = np.where(imin > 0, imin.astype(np.int32).view(F32), F32(0.0))
    stot = np.asarray(Sn, F32).sum(dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        gmax = np.where(vmax > 0, np.minimum(np.ceil(vmax * scale), scale), 0).astype(np.int64)
        gmin = np.where(vmin > 0, np.minimum(np.ceil(vmin * scale), scale + 1), 0).astype(np.int64)
    lo = np.where(gmin >= 2, gmin - 1, 0)
    hi = np.where(gmax < 1, 1, gmax)
    reset = (lo > 0) & (not stot > F32(kappa))
    lo, hi = np.where(reset, 0, lo), np.where(reset, 1, hi)
    over = lo >= top
    lo, hi = np.where(over, top - 1, lo), np.where(over, top, hi)
    hi = np.where(hi <= lo, lo + 1, hi)
    return np.where(nanc, 0, lo), np.where(nanc, top, hi)


# The shapes the GPU case table (tests/test_gpu_consensus_forms.py) runs, half
# on either stake grid; tests/test_consensus_cases_host.py proves the input
# conditions on every one of them.
SHAPES = (
    (13, 36, "u24"), (40, 132, "u20"), (70, 260, "u24"), (200, 132, "u20"), (70, 262, "u20"),
    (300, 68, "u24"), (300, 67, "u20"), (1100, 96, "u20"), (130, 520, "u24"),
    # every row real (no padding rows in the wave forms): the bracket's lower end is live
    (16, 36, "u20"), (64, 132, "u24"), (256, 260, "u20"),
    # one validator holds all the stake
    (70, 260, "single"), (300, 68, "single"),
)
