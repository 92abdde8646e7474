"""The conditions tests/test_gpu_consensus_forms.py relies on, proved on the CPU.

For every shape of consensus_cases.SHAPES:
  * the big-integer bisection (consensus_cases.bisect_exact) and the oracle's
    fp32 bisection (oracle.yuma_oracle.consensus) agree bit for bit, raw and
    quantised, on every epoch (the non-finite one included), kappa and
    precision -- no column is excluded and no tie window is used;
  * stakes are exact multiples of 2^-24 after normalisation and total <= 1,
    weights are integers whose rows sum to a power of two;
  * every column family does what it is there for, read from the reference's
    own trace (the stake above each midpoint, a staked validator on the
    midpoint) and the brackets as the kernels form them;
  * at the default precision, moving the raw consensus of any family column
    by one grid point, up or down, changes the quantised C. For the 10- and
    24-step grids the share of such columns is printed (pytest -s), not
    asserted, and so is the single-staker shapes' share: there sum(C_raw) is
    about 1 (the staker's whole row), one grid step is half a level."""

import numpy as np
import pytest

import consensus_cases as cc
from oracle import yuma_oracle as orc

F32 = np.float32
SHAPES = cc.SHAPES
FAMILIES = [s for s in SHAPES if s[2] != "single"]
ids = lambda s: f"V{s[0]}-M{s[1]}-{s[2]}"  # noqa: E731


def normalised(inp, e):
    return cc.normalise(inp.W[e]), cc.normalise_stake(inp.S[e])


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_the_two_references_agree(shape):
    inp = cc.build(*shape)
    assert inp.W.shape[0] == 4
    kappas = cc.KAPPAS + ((0.0, 1.0) if shape[0] in (16, 64, 300) else ())
    for e in range(4):
        Wn, Sn = normalised(inp, e)
        for kappa in kappas:
            for precision in cc.PRECISIONS:
                top = 1 << orc.bisect_iterations(precision)
                raw = np.array([k / top for k in cc.bisect_exact(Wn, Sn, kappa, precision)], dtype=np.float64)
                ref = orc.consensus(Wn, Sn, kappa, precision, as_double=True)
                tag = f"epoch {e} kappa {kappa} precision {precision}"
                np.testing.assert_array_equal(raw, ref, err_msg=tag)
                for dbl in (False, True):
                    np.testing.assert_array_equal(
                        cc.consensus_exact(Wn, Sn, kappa, precision, dbl),
                        orc.quantise(ref if dbl else ref.astype(F32), dbl), err_msg=tag)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_reference_is_the_oracle_run(shape):
    """reference_C, what the GPU tests compare with, is oracle.run's C on the
    finite epochs (Yuma 3 in fp32, Yuma 0 in fp64)."""
    inp = cc.build(*shape)

    class Cfg:
        kappa, consensus_precision, liquid_alpha = 0.5, 100000, False
        bond_alpha, decay_rate, capacity_alpha, bond_penalty = 0.1, 0.1, 0.1, 1.0

    for version, dbl in (("Yuma 3 (Rhef)", False), ("Yuma 0 (subtensor)", True)):
        ref = orc.run(version, inp.W[:2], inp.S[:2], Cfg)
        np.testing.assert_array_equal(cc.reference_C(*shape, 0.5, 100000, dbl)[:2], ref["C"])


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_stakes_and_weights_are_exact(shape):
    inp = cc.build(*shape)
    V, M, kind = shape
    assert inp.W.shape == (4, V, M) and inp.S.shape == (4, V)
    for e in range(4):
        S = inp.S[e].astype(np.float64)
        assert (S == np.floor(S)).all() and S.sum() == {"u24": 2**24, "u20": 2**20, "single": 2**24}[kind]
        Sn = cc.normalise_stake(inp.S[e])
        units = cc.stake_units(Sn)  # asserts multiples of 2^-24, total <= 1
        assert sum(units) == 2**24 and units.count(0) >= 2
        assert kind != "single" or sorted(units)[-2:] == [0, 2**24]
    for e in (0, 1):
        W = inp.W[e].astype(np.float64)
        assert (W == np.floor(W)).all() and W.min() >= 0 and W.max() <= 65535
        rs = W.sum(axis=1)
        assert (rs == (cc.ROW if e == 0 else cc.ONE_ROW)).all()
        assert (F32(rs) + F32(1e-6) == F32(rs)).all()
        np.testing.assert_array_equal(cc.normalise(inp.W[e]).astype(np.float64), W / rs[:, None])
    # on the 17-step grid, values off the 10-step grid on both sides of a grid point
    g = inp.W[0].astype(np.int64)
    assert (g % 128 == 1).any() and (g % 128 == 127).any()
    # the non-finite epoch: single entries, their rows poisoned as the reference does
    W2, Wn2 = inp.W[2], cc.normalise(inp.W[2])
    nf = inp.nonfinite
    assert np.isnan(W2[nf["nan"]]) and W2[nf["+inf"]] == np.inf and W2[nf["-inf"]] == -np.inf
    assert W2[nf["negative"]] == -5 and W2[nf["-0.0"]] == 0 and np.signbit(W2[nf["-0.0"]])
    assert (~np.isfinite(W2)).sum() == 3
    single = [nf[k] for k in ("nan", "+inf", "-inf", "negative", "-0.0")]
    assert len({r for r, _ in single}) == 5
    assert np.isnan(Wn2[nf["nan"][0]]).all()
    for k in ("+inf", "-inf"):
        r, c = nf[k]
        assert np.isnan(Wn2[r, c]) and (np.delete(Wn2[r], c) == 0).all()
    assert Wn2[nf["negative"]] == F32(-5.0 / cc.ROW) and np.signbit(Wn2[nf["-0.0"]])
    finite_rows = np.isfinite(W2).all(axis=1)
    assert (W2[finite_rows].astype(np.float64).sum(axis=1) == cc.ROW).all()
    # epoch 3: a column above 1.0 in every row (lo_c >= top), paid for by negative fillers; sums stay exact
    W3, Wn3, over = inp.W[3].astype(np.float64), cc.normalise(inp.W[3]), nf["over"][1]
    assert (W3 == np.floor(W3)).all() and (W3.sum(axis=1) == cc.ROW).all() and np.abs(W3).sum(axis=1).max() < 2**24
    np.testing.assert_array_equal(Wn3.astype(np.float64), W3 / cc.ROW)
    assert (Wn3[:, over] == F32(1 + 2.0**-14)).all()
    assert set(np.nonzero(W3 < 0)[1]) <= set(inp.fillers)
    for precision in cc.PRECISIONS:
        iters = orc.bisect_iterations(precision)
        l3, h3 = cc.bracket(Wn3, cc.normalise_stake(inp.S[3]), 0.5, iters)
        assert l3[over] == 2**iters - 1 and h3[over] == 2**iters
        assert cc.bisect_exact(Wn3, cc.normalise_stake(inp.S[3]), 0.5, precision)[over] == 2**iters


def test_placement_over_the_table():
    """Every shape has family columns in its last, partly filled tile; over
    the table every family (a..f) gets there, and in the one-tile and the
    32-column shapes all of them at once. A lane quad (4 aligned columns) with
    two families exists in every shape, and fnarrow / fwide share one."""
    reached = set()
    for shape in SHAPES:
        inp = cc.build(*shape)
        assert len(inp.last_tile) < 64
        here = {cc.FAMILY[n] for n, cols in inp.columns.items() for c in cols if c in inp.last_tile}
        assert here, shape
        if len(inp.last_tile) >= 32:
            assert here == set("abcdef"), shape
        reached |= here
        quads = {}
        for n, cols in inp.columns.items():
            for c in cols:
                quads.setdefault(c // 4, set()).add(cc.FAMILY[n])
        assert any(len(f) > 1 for f in quads.values())
        for a, b in zip(inp.columns["fnarrow"], inp.columns["fwide"]):
            assert a // 4 == b // 4 and len(quads[a // 4]) > 1  # ... next to another family
        assert inp.one_col in inp.last_tile
        assert set(inp.columns) == set(cc.NAMES)
    assert reached == set("abcdef")


@pytest.mark.parametrize("shape", FAMILIES, ids=ids)
def test_every_family_occurs_as_intended(shape):
    inp = cc.build(*shape)
    V, M, kind = shape
    Wn, Sn = normalised(inp, 0)
    units = np.array(cc.stake_units(Sn), dtype=np.int64)
    staked = units > 0
    U = inp.unit
    traces, kstar = {}, {}
    for kappa in cc.KAPPAS:
        for precision in cc.PRECISIONS:
            tr = []
            kstar[kappa, precision] = cc.bisect_exact(Wn, Sn, kappa, precision, trace=tr)
            traces[kappa, precision] = tr

    def seen(kappa, precision, col, key):
        return [step[key][col] for step in traces[kappa, precision]]

    # (a) the stake above a probed midpoint is exactly floor(fp32(kappa) 2^24) units, and one unit more / less
    for kappa in cc.KAPPAS:
        kk = cc.kappa_units(kappa)
        tie = kk // U * U  # "u20": 0.3 and 0.7 have no exact tie on multiples of 16 units
        assert kind == "u20" or tie == kk
        assert kappa != 0.5 or tie == kk
        tag = "a" + str(kappa)[-1]
        for precision in cc.PRECISIONS:  # the tie is probed on all three grids
            for c in inp.columns[tag]:
                assert tie in seen(kappa, precision, c, "units"), (tag, c)
            for c in inp.columns[tag + "+"]:
                assert tie + U in seen(kappa, precision, c, "units"), (tag, c)
            for c in inp.columns[tag + "-"]:
                assert tie - U in seen(kappa, precision, c, "units"), (tag, c)
        # one stake unit moves the result by one grid point of the default grid
        top = 1 << 17
        for c0, c1 in zip(inp.columns[tag], inp.columns[tag + "+"]):
            assert kstar[kappa, 100000][c0] == cc.T and kstar[kappa, 100000][c1] == cc.T + 1
        for c in inp.columns[tag + "-"]:
            assert kstar[kappa, 100000][c] <= cc.T
        assert top == 1 << orc.bisect_iterations(100000)
    # (b) a staked validator's Wn equals a probed midpoint, on every grid, and decides the column
    for kappa in cc.KAPPAS:
        for precision in cc.PRECISIONS:
            for c in inp.columns["b"]:
                assert any(seen(kappa, precision, c, "on_grid")), (kappa, precision, c)
        for c in inp.columns["b"]:
            k = kstar[kappa, 100000][c]
            assert (staked & (Wn[:, c] == F32(k / 2**17))).any()
    # at the default precision every family column with stake on it is decided by a strict `>` on a grid point
    for c in inp.targeted:
        assert any(seen(0.5, 100000, c, "on_grid")) or kstar[0.5, 100000][c] == 1
    # (c) zero-stake extremes
    for c in inp.columns["cmax"]:
        top_rows = Wn[:, c] == Wn[:, c].max()
        assert not staked[top_rows].any() and Wn[staked, c].max() < Wn[:, c].max()
    for c in inp.columns["cmin"]:
        low_rows = Wn[:, c] == Wn[:, c].min()
        assert not staked[low_rows].any() and Wn[staked, c].min() > Wn[:, c].min()
    # (d) low total stake: the lowest grid point on every grid
    for c in inp.columns["d"]:
        assert 0 < units[Wn[:, c] > 0].sum() <= min(cc.kappa_units(k) for k in cc.KAPPAS)
        assert all(k[c] == 1 for k in kstar.values())
    # (e) degenerate columns
    for c in inp.columns["e0"]:
        assert (Wn[:, c] == 0).all() and all(k[c] == 1 for k in kstar.values())
    for c in inp.columns["e1"]:
        assert np.count_nonzero(Wn[:, c]) == 1
    lo, hi = cc.bracket(Wn, Sn, 0.5, 17)
    for c in inp.columns["esame"]:
        assert (Wn[:, c] == Wn[0, c]).all() and Wn[0, c] > 0 and hi[c] - lo[c] <= 1
        assert all(k[c] == cc.T for (_, p), k in kstar.items() if p == 100000)
    Wn1, Sn1 = normalised(inp, 1)
    assert (Wn1[:, inp.one_col] == F32(1.0)).all() and (np.delete(Wn1, inp.one_col, axis=1) == 0).all()
    for kappa in cc.KAPPAS:
        for precision in cc.PRECISIONS:
            iters = orc.bisect_iterations(precision)
            k1 = cc.bisect_exact(Wn1, Sn1, kappa, precision)
            assert k1[inp.one_col] == 1 << iters and sum(k1) == (1 << iters) + M - 1
            l1, h1 = cc.bracket(Wn1, Sn1, kappa, iters)
            assert l1[inp.one_col] == (1 << iters) - 1  # lo_c >= top
    # (f) mixed bracket widths in one lane quad, on the grids where a histogram can take 64 points
    for precision in (100000, 10000000):
        lo, hi = cc.bracket(Wn, Sn, 0.5, orc.bisect_iterations(precision))
        if precision == 100000:
            for a, b in zip(inp.columns["fnarrow"], inp.columns["fwide"]):
                assert hi[a] - lo[a] <= 8 and hi[b] - lo[b] >= 64 and a // 4 == b // 4 and a // 16 == b // 16
            # whole waves (16 columns) of brackets of <= 8 grid points exist beside them (the fall-back)
            w = (hi - lo)[: M // 16 * 16].reshape(-1, 16)
            assert M < 64 or ((w <= 8).all(axis=1)).any()
            # ... and a wave with a lane quad of such brackets next to wider ones (no fall-back for that wave)
            q = w.reshape(w.shape[0], 4, 4)
            assert M < 64 or (((q <= 8).all(axis=2)).any(axis=1) & (w > 8).any(axis=1)).any()


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_one_grid_point_changes_the_quantised_consensus(shape):
    inp = cc.build(*shape)
    Wn, Sn = normalised(inp, 0)
    for precision in (100000, 1000, 10000000):
        top = 1 << orc.bisect_iterations(precision)
        for kappa in cc.KAPPAS:
            k = cc.bisect_exact(Wn, Sn, kappa, precision)
            raw = np.array([x / top for x in k], dtype=np.float64)
            base = orc.quantise(raw.astype(F32), False)
            moved = 0
            for c in inp.targeted:
                for d in (-1, 1):
                    r = raw.copy()
                    r[c] = (k[c] + d) / top
                    moved += not np.array_equal(orc.quantise(r.astype(F32), False), base)
            n = 2 * len(inp.targeted)
            print(f"[sensitivity] {ids(shape)} kappa {kappa} precision {precision}: sum(C_raw) = {raw.sum():.4f}, "
                  f"{moved} / {n} one-point moves change C")
            if precision == 100000 and shape[2] != "single":
                assert raw.sum() <= 0.5
                assert moved == n
