"""tests/division_cases.py proves its claims here (no GPU): the row sums of
every shape do not depend on the summation order, most quotients of the rows
inside the guard are inexact, every family is on the side of row_div's guard
and of screen_ok that its name says, a Yuma 4 epoch with bond_alpha = 0.5 shows
the bits of Wn, a pair stake leaves at most two terms per column sum, and the
case table of tests/test_gpu_division_forms.py names the bond scan that
engine.scan_plan reports."""

from __future__ import annotations

from fractions import Fraction

import numpy as np
import pytest

import division_cases as dc
from oracle import yuma_oracle as orc

F32 = np.float32
SHAPES = dc.SHAPES
IDS = [f"{v}x{m}" for v, m in SHAPES]


def forward(x):
    return np.cumsum(x, dtype=F32)[-1]


def kernel_order(x):
    """k_rowsum: 256-miner chunks; per chunk the quad sums ((x0 + x1) + x2) + x3
    of the 64 lanes, the lanes' balanced (xor butterfly) tree, the chunks added
    in order to a sum that starts at +0. The WIDE form (rows of 64 chunks and
    more) parks the chunk sums and adds them in the same order."""
    M = x.size
    pad = np.zeros(-(-M // 256) * 256, dtype=F32)
    pad[:M] = x
    q = pad.reshape(-1, 64, 4)
    q = ((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3]
    while q.shape[1] > 1:
        q = q[:, 0::2] + q[:, 1::2]
    acc = F32(0.0)
    for c in q[:, 0]:
        acc = F32(acc + c)
    return acc


def wide_order(x):
    """The WIDE form literally: chunk k by wave k % 4 into qs[k], one lane adds
    qs[0 .. nc - 1] in order."""
    M = x.size
    nc = -(-M // 256)
    pad = np.zeros(nc * 256, dtype=F32)
    pad[:M] = x
    qs = np.zeros(nc, dtype=F32)
    for wave in range(4):
        for k in range(wave, nc, 4):
            q = pad[k * 256:(k + 1) * 256].reshape(64, 4)
            q = ((q[:, 0] + q[:, 1]) + q[:, 2]) + q[:, 3]
            for o in (1, 2, 4, 8, 16, 32):  # x + shfl_xor(x, o)
                q = q + q[np.arange(64) ^ o]
            assert (q == q[0]).all()
            qs[k] = q[0]
    return forward(np.concatenate([[F32(0.0)], qs]).astype(F32))


@pytest.mark.parametrize("V,M", SHAPES, ids=IDS)
def test_row_sums_do_not_depend_on_the_order(V, M):
    inp = dc.build(V, M)
    rng = np.random.default_rng(V * 100003 + M)
    epochs = [(inp.W[0], "tame"), (inp.W[1], "signed"), (inp.W_plain, "plain-only")]
    for W, name in epochs:
        ints = (W == np.floor(W)).all(axis=1) & (np.abs(W).sum(axis=1, dtype=np.float64) < 2.0 ** 52)
        for v in range(V):
            x = W[v]
            exact = Fraction(int(x.astype(np.float64).sum())) if ints[v] else dc.exact_sum(x)
            want = orc._round_f32(exact)
            sums = {"forward": forward(x), "reverse": forward(x[::-1]), "numpy": x.sum(dtype=F32),
                    "kernel": kernel_order(x), "shuffled": forward(x[rng.permutation(M)]),
                    "ascending": forward(np.sort(x)), "by magnitude": forward(x[np.argsort(-np.abs(x))])}
            if M >= 16384:
                sums["wide"] = wide_order(x)
            for order, got in sums.items():
                assert got.view(np.uint32) == want.view(np.uint32) or (got == 0 and want == 0), (
                    f"{name} row {v} ({inp.family_of(0)[v]}): the {order} sum {got!r} is not RN(exact) {want!r}")
    # the non-finite epoch: the rows without a non-finite entry are plain
    bad = {r for n in dc.NONFINITE for r in inp.rows[n]}
    for v in range(V):
        if v not in bad:
            x = inp.W[2, v]
            assert forward(x) == x.sum(dtype=F32) == kernel_order(x) == F32(int(x.astype(np.float64).sum()))


@pytest.mark.parametrize("V,M", SHAPES, ids=IDS)
def test_most_quotients_inside_the_guard_are_inexact(V, M):
    """plain, lo-in and hi-near rows: w / rs is no fp32 for more than half of the
    nonzero weights, so exact divisions alone cannot pass. hi-in's divisor is
    2^60, a power of two: its quotients are exact by construction, and hi-near is
    the row that holds the upper side of the guard with inexact quotients."""
    inp = dc.build(V, M)
    W = inp.W[0]
    rs = dc.row_sums(W).astype(np.float64)
    Wn = dc.normalise(W)
    for name in ("plain", "lo-in", "hi-near", "hi-in"):
        for v in inp.rows.get(name, ()):
            nz = W[v] != 0
            exact = np.array([Fraction(float(a)) / Fraction(float(rs[v])) == Fraction(float(q))
                              for a, q in zip(W[v][nz].tolist(), Wn[v][nz].tolist())])
            if name == "hi-in":
                assert rs[v] == 2.0 ** 60 and exact.all()
            else:
                assert np.log2(rs[v]) % 1 != 0, f"row {v} ({name}): the divisor is a power of two"
                assert (~exact).mean() > 0.5, f"row {v} ({name}): {(~exact).mean():.2f} inexact"


@pytest.mark.parametrize("V,M", SHAPES, ids=IDS)
def test_every_family_is_on_its_side_of_the_guard(V, M):
    inp = dc.build(V, M)
    W = inp.W[0]
    rs = dc.row_sums(W)
    fast, scr, dok = dc.fast_row(W), dc.screen_ok(W), dc.row_div_ok(rs)
    slow = dc.slow_elements(W).any(axis=1)
    assert np.array_equal(fast, ~slow)  # the row screen is the elementwise guard, row by row
    for name, rows in inp.rows.items():
        if name not in dc.TAME + ("plain",):
            continue
        for v in rows:
            assert bool(fast[v]) == (name in dc.INSIDE), f"row {v} ({name}): fast {fast[v]}"
    nzmin = lambda v: np.abs(W[v][W[v] != 0]).min()
    for v in inp.rows["lo-in"]:
        assert nzmin(v) == dc.LO and scr[v] and dok[v]
    for v in inp.rows["lo-out"]:
        assert nzmin(v) == np.nextafter(dc.LO, F32(0)) and not scr[v] and dok[v]
        assert dc.slow_elements(W)[v].sum() == 1  # that one weight alone
    for v in inp.rows["hi-in"]:
        assert W[v].max() == dc.HI and rs[v] == dc.HI and scr[v] and dok[v]
    for v in inp.rows["hi-out"]:
        assert W[v].max() == np.nextafter(dc.HI, F32(np.inf)) and not scr[v] and not dok[v]
    for v in inp.rows.get("hi-sum", ()):
        assert rs[v] == F32(2.0 ** 61) and scr[v] and not dok[v]
    for v in inp.rows.get("hi-near", ()):
        assert 2.0 ** 59 <= rs[v] < 2.0 ** 60 and scr[v] and dok[v]
    for v in inp.rows["down"]:
        assert W[v].max() < dc.LO and not scr[v] and dok[v] and abs(float(rs[v]) - 1e-6) < 1e-9
    for v in inp.rows["up"]:
        assert rs[v] > dc.HI and W[v].max() <= dc.HI and scr[v] and not dok[v]
    for v in inp.rows.get("subnormal", ()):
        assert 0 < nzmin(v) < np.finfo(F32).tiny and not scr[v] and dok[v]
    Wn = dc.normalise(W)
    for v in inp.rows.get("tiny-q", ()):
        q = Wn[v][W[v] != 0]
        assert (q == 0).any() and ((q > 0) & (q < np.finfo(F32).tiny)).any() and not dok[v]
    for v in inp.rows.get("zero", ()):
        assert not W[v].any() and not np.signbit(W[v]).any() and rs[v] == dc.EPS
    for v in inp.rows.get("mzero", ()):
        assert (np.signbit(W[v]) & (W[v] == 0)).sum() >= 2 and (W[v] >= 0).all()
        assert np.signbit(Wn[v][np.signbit(W[v])]).all()  # IEEE keeps the sign
    # the signed epoch
    W1, rs1 = inp.W[1], dc.row_sums(inp.W[1])
    for v in inp.rows["neg"]:
        assert rs1[v] < 0 and (W1[v] <= 0).all() and dc.fast_row(W1)[v]
    for v in inp.rows["cancel"]:
        q = dc.normalise(W1)[v]
        assert rs1[v] == dc.EPS and (W1[v] < 0).any() and np.abs(q).max() > 1e8 and dc.fast_row(W1)[v]
    # every aligned group of four rows (a k_rowsum block, the smallest tile) holds a plain row
    fam = inp.family_of(0)
    for g in range(0, V - V % 4, 4):
        assert any(fam[v] == "plain" for v in range(g, g + 4)), g
    assert fam[0] != "plain" and fam[V - 1] != "plain"
    for b in dc.BOUNDARIES:
        if b < V - 1:
            assert fam[b - 1] != "plain" and fam[b] != "plain"
    # the non-finite epoch
    for name, pred in (("nan", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
        (v,) = inp.rows[name]
        assert pred(inp.W[2, v]).sum() == 1 and np.isfinite(inp.W[2, v]).sum() == M - 1
    # the stakes
    for e in range(3):
        Sn = inp.S[e] / inp.S[e].sum(dtype=F32)
        assert float(inp.S[e].sum(dtype=F32)) == 2.0 ** 16 and (Sn * 2.0 ** 16 == inp.S[e]).all()
        assert (inp.S[e][list(inp.edge_rows)] > 0).all() and (inp.S[e] == 0).any()


@pytest.mark.parametrize("V,M", SHAPES, ids=IDS)
def test_a_yuma4_epoch_shows_the_bits_of_wn(V, M):
    """Observation 2, one epoch of each kind and both two-epoch orders; C's
    normalising sum is exact as well (multiples of 2^-17 totalling < 2^7)."""
    for order in ((0,), (1,), (2,), (0, "plain"), ("plain", 0)):
        ref = dc.reference(V, M, "spread", order)
        inp = dc.build(V, M)
        W, _ = dc.epochs_of(inp, order)
        Wn = dc.normalise(W)
        assert np.array_equal(ref["Wn"].view(np.int32), Wn.view(np.int32))
        B0 = dc.yuma4_bits(Wn[0])
        assert np.array_equal(ref["B"][0].view(np.int32), B0.view(np.int32)), order
        if order[0] in (0, "plain"):
            # the halving is exact wherever it cannot underflow
            big = np.abs(Wn[0]) >= 2 * np.finfo(F32).tiny
            assert np.array_equal((B0 * F32(2))[big & (B0 < 1)], Wn[0][big & (B0 < 1)])
        if len(order) == 2:
            B1 = dc.yuma4_bits(Wn[1], 0.5, B0)
            assert np.array_equal(ref["B"][1].view(np.int32), B1.view(np.int32)), order
    ref = dc.reference(V, M, "spread", (0,))
    inp = dc.build(V, M)
    raw = orc.consensus(ref["Wn"][0], inp.S[0] / inp.S[0].sum(dtype=F32), 0.5, 100000, False)
    assert (raw * 2.0 ** 17 == np.floor(raw * 2.0 ** 17)).all() and raw.astype(np.float64).sum() < 2.0 ** 7
    assert raw.max() > 0


pairs = dc.pairs


PAIR_SHAPES = sorted({(c.V, c.M) for c in dc.CASES if c.kind in ("col", "y3pair")})


@pytest.mark.parametrize("V,M", PAIR_SHAPES, ids=[f"{v}x{m}" for v, m in PAIR_SHAPES])
def test_pair_stakes_leave_two_terms_per_column(V, M):
    """... and the rank pass's column screen (csr) passes on some columns of every
    run and fails on some columns of the lo-in, lo-out and tiny-q runs, so both
    branches of the csb path of k_bonds_elem are taken."""
    seen = {}
    for name, i, j in pairs(V, M):
        inp = dc.build(V, M, ("pair", i, j))
        Sn = inp.S[0] / inp.S[0].sum(dtype=F32)
        assert Sn[i] == Sn[j] == 0.5 and np.count_nonzero(Sn) == 2
        for version in ("Yuma 0 (subtensor)", "Yuma 1 (paper)", "Yuma 2 (Adrian-Fish)"):
            ref = dc.reference(V, M, ("pair", i, j), (0,), version)
            num = ref["B"][0]  # the normalised bonds: nonzero only where S * W_b is
            assert (np.count_nonzero(np.nan_to_num(num), axis=0) <= 2).all(), (name, version)
            assert not np.isnan(num).any()
        Wn = dc.reference(V, M, ("pair", i, j), (0,), "Yuma 1 (paper)")["Wn"][0]
        ok = dc.csr_ok(Sn[:, None] * Wn)  # bond_penalty 0: W_b is Wn
        live = np.count_nonzero(Sn[:, None] * Wn, axis=0) > 0
        seen[name] = (bool((ok & live).any()), bool((~ok & live).any()))
    assert all(p for p, _ in seen.values()), seen
    for name in ("lo-in", "lo-out", "tiny-q"):
        assert name not in seen or seen[name][1], (name, seen)


@pytest.mark.parametrize("V,M", SHAPES, ids=IDS)
def test_the_rare_branches_are_reached(V, M):
    """What the GPU cases rely on without being able to see it. The screened
    scans' NaN reciprocal and the `__any(slow)` redo: every shape has rows that
    fail the screen beside rows that pass it, in one 4-row group. rq4.w (the sweep
    scan's negative-weight branch): the signed epoch has rows with a weight below
    -0. min(Wn, C) meets a -0 under C = +0 in the mzero family alone (where the
    quantised C of a column is 0); no other epoch has such a tie."""
    inp = dc.build(V, M)
    fast = dc.fast_row(inp.W[0])
    assert any(fast[g:g + 4].any() and not fast[g:g + 4].all() for g in range(0, V, 4))
    assert (~fast).sum() >= 5 and fast[inp.rows["plain"]].all()
    assert all((inp.W[1][v] < 0).any() for n in dc.SIGNED for v in inp.rows[n])
    assert not (inp.W_plain < 0).any() and not np.signbit(inp.W_plain).any()
    zc = dc.zero_column(M)
    assert not inp.W[0][:, zc].any() and not inp.W_plain[:, zc].any()
    for e in (0, 1, 2):
        ref = dc.reference(V, M, "spread", (e,), "Yuma 3 (Rhef)")
        Wn, C = ref["Wn"][0], ref["C"][0]
        tie = np.signbit(Wn) & (Wn == 0) & (C == 0)[None, :]
        rows = set(np.nonzero(tie.any(axis=1))[0].tolist())
        assert rows <= (set(inp.rows.get("mzero", ())) if e == 0 else set()), (e, rows)


@pytest.mark.parametrize("case", dc.CASES, ids=[c.id for c in dc.CASES])
def test_case_table_matches_the_dispatch(case):
    """engine.scan_plan (host only) reports the bond scan named for the case; V
    sits in the range of DESIGN.md 2.0 for the named rank kernel."""
    from yuma_simulation._internal import engine

    assert (case.V, case.M) in dc.SHAPES
    kw = case.kw
    E = 2 if "hist_stride" in kw else 1
    N = 4 if case.kind == "grp" else 1
    plan = engine.scan_plan(case.variant, N, E, case.V, case.M, case.hist, case.want,
                            shared_inputs=case.kind == "grp", hist_stride=kw.get("hist_stride", 1),
                            hist_first=kw.get("hist_first"), hist_bf16="hist_dtype" in kw, sched="sched" in kw)
    assert (plan.form, plan.shape, plan.rq) == case.scan, plan
    assert plan.vector_form == (case.M % 4 == 0) and plan.hist == case.hist
    assert plan.hs == ("hist_stride" in kw) and plan.hist_bf16 == ("hist_dtype" in kw) and plan.sc == ("sched" in kw)
    assert case.rank == dc.rank_kernel(case)
    assert case.V <= 1024 or "BIGV" in case.rank
