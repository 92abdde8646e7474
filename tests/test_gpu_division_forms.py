"""Every kernel form that divides (gpu marker) on the edge rows of
tests/division_cases.py, every element compared bit for bit.

The inputs' row sums do not depend on the summation order and the stakes are
exact (tests/test_division_cases_host.py proves both, and that every row family
sits on its side of div_fast's guard and of k_rowsum's screen), so the only
freedom an implementation has is the division itself: Wn, Wc, C and the bonds
have to equal IEEE fp32 division, through the numpy oracle, on every element of
the tame and the signed epoch, and on the non-finite epoch NaN has to stand at
the same positions with equal bits elsewhere. No mask, no tie window.

division_cases.CASES names, per case, the rank kernel and the bond scan the
shape reaches (the host test holds the table to engine.scan_plan). Kinds:
  wn      Yuma 3 with Wn / Wc (/ R / P) requested: the materialising rank forms
  wn2     Yuma 2 over [tame, plain-only]: epoch 1 clips the previous slice's Wn
  bonds   Yuma 4, bond_alpha 0.5, zero bonds: B = min(0.5 Wn, 1) shows Wn's bits
          as the element-wise scans form it; one epoch of each kind and the
          two-epoch orders [tame, plain-only] / [plain-only, tame]; the history,
          B_final, B_watch or B_rows, whichever the case's form writes
  grp     the same through a shared-input sweep of four scenarios, two of them
          bond_alpha 0.25, against the replicated run and the oracle
  y3pair  Yuma 3 under a pair stake (normalised stakes 1/2)
  col     Yuma 0 / 1 / 2 (bond_penalty 0) under pair stakes, one run per edge
          family paired with a plain row: S W_b / column sum
On every case C equals the oracle bit for bit and the YUMA_FLAG_NO_HIST run
equals the histogram run; on the tame epoch R, I and Dn (sums whose order is
free) lie within the suite's RTOL / ATOL_FRAC.

One thing is not the division's: min(-0, +0). Where a weight is -0, Wn is -0
and every materialising kernel reproduces that bit (Wn is compared strictly on
every row; the Yuma 4 bonds cannot show it, 0 + (-0) is +0). W_c = min(Wn, C)
with C = +0 is a tie of two zeros: numpy and torch return the second operand
(+0), the kernels' v_minimum3_f32 orders -0 below +0 and returns -0 (observed
bits 0x80000000 against 0x00000000), and Yuma 0 / 1 / 2
carry that zero's sign through S W_c into the bonds. That is a property of the
instruction, and it concerns one family, mzero (division_cases.tie_rows finds
the rows from the reference; the host test proves that no other family and no
other epoch has such a tie). So every case whose run has such a tie is two
items: `all` compares W_c and the column bonds on every row but the mzero rows,
and everything else on every row; `mzero` compares them on the mzero rows, bit
for bit, and is a strict expected failure."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import division_cases as dc
from conftest import ATOL_FRAC, RTOL, assert_close  # noqa: F401
from division_cases import Y0, Y1, Y2, Y3, Y4

pytestmark = pytest.mark.gpu

from yuma_simulation._internal import engine  # noqa: E402
from yuma_simulation._internal.yumas import SimulationHyperparameters, YumaConfig, YumaParams  # noqa: E402

ORDERS = ((0,), (1,), (2,), (0, "plain"), ("plain", 0))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "gpu tests need a ROCm GPU"
    engine.load_library()
    yield
    torch.cuda.empty_cache()


def params(variant, alpha=0.5, nohist=False):
    cfg = YumaConfig(simulation=SimulationHyperparameters(bond_penalty=0.0), yuma_params=YumaParams(bond_alpha=alpha))
    p = engine.make_params(variant, cfg)
    if nohist:
        p.flags |= engine.FLAG_NO_HIST
    return p


def ref_of(case, stake, order, alpha=0.5):
    cfg = YumaConfig(simulation=SimulationHyperparameters(bond_penalty=0.0), yuma_params=YumaParams(bond_alpha=alpha))
    assert (cfg.kappa, cfg.consensus_precision, cfg.capacity_alpha, cfg.decay_rate, cfg.liquid_alpha) == (
        dc.Params.kappa, dc.Params.consensus_precision, dc.Params.capacity_alpha, dc.Params.decay_rate, False)
    return dc.reference(case.V, case.M, stake, order, dc.VERSION[case.variant], bond_alpha=alpha)


def same(got, want, tag, fam=None, nonfinite=False, rows=None):
    """Every element: equal bits (nonfinite: NaN at the same positions, equal
    bits elsewhere). fam: row -> family, for the message (rows on axis -2).
    rows: compare these rows (axis -2) only."""
    g = got.detach().float().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float32)
    w = np.asarray(want, np.float32)
    assert g.shape == w.shape, f"{tag}: shape {g.shape} != {w.shape}"
    if rows is not None:
        g, w = np.ascontiguousarray(np.take(g, rows, axis=-2)), np.ascontiguousarray(np.take(w, rows, axis=-2))
        fam = {k: fam[r] for k, r in enumerate(rows)} if fam else None
    gb, wb = g.view(np.int32), w.view(np.int32)
    bad = gb != wb
    if nonfinite:
        bad &= ~(np.isnan(g) & np.isnan(w))
    if bad.any():
        at = np.argwhere(bad)
        rows = sorted({int(i[-2]) for i in at}) if g.ndim >= 2 and fam else []
        first = [(tuple(int(x) for x in i), float(g[tuple(i)]), float(w[tuple(i)]), hex(int(gb[tuple(i)]) & 0xFFFFFFFF),
                  hex(int(wb[tuple(i)]) & 0xFFFFFFFF)) for i in at[:6]]
        raise AssertionError(f"{tag}: {len(at)} elements differ; rows (family) "
                             f"{[(r, fam[r]) for r in rows[:12]] if fam else '-'}; (index, got, want, bits) {first}")


def split_rows(case, part, stake="spread"):
    """The rows an item compares W_c and the column bonds on: `mzero` the rows
    with a min(-0, +0) tie, `all` every other row (every row where the run has
    no tie)."""
    tie = list(dc.tie_rows(case, stake))
    if part == "mzero":
        return tie
    return [v for v in range(case.V) if v not in tie] if tie else None


def close(got, want, what):
    assert_close(got.cpu().numpy() if isinstance(got, torch.Tensor) else got, want, what=what)


def tensors(case, stake, order):
    inp = dc.build(case.V, case.M, stake)
    W, S = dc.epochs_of(inp, order)
    dev = engine.device()
    return inp, torch.from_numpy(W[:, None].copy()).to(dev), torch.from_numpy(S[:, None].copy()).to(dev)


def fam_of(inp, order):
    if len(order) == 2:
        return inp.family_of(0)
    return inp.family_of(order[0])


def run_kw(case, inp, E):
    """run()'s keywords from the case's options."""
    kw = {}
    for k, v in case.opts:
        if k == "sched":
            kw[k] = list(range(E))
        elif k == "hist_dtype":
            kw[k] = torch.bfloat16
        elif k == "watch":
            kw[k] = sorted(set(range(0, case.M, 7)) | {case.M - 1})
        elif k == "watch_rows":
            kw[k] = list(inp.edge_rows) + inp.rows["plain"][:2]
        elif k in ("resets", "row_resets"):
            kw[k] = torch.zeros((0, 4), dtype=torch.int32)
        else:
            kw[k] = v
    return kw


def check_common(case, res, alt, ref, order, tag, n=0):
    """C against the oracle, the bisection run against the histogram run, and on
    finite input the order-dependent sums within the suite's tolerance."""
    nonfinite = 2 in order
    same(res.C[:, n], ref["C"], f"{tag} C", nonfinite=nonfinite)
    if alt is not None:
        for k in ("C", "Dn", "I", "B_final"):
            same(getattr(alt, k), getattr(res, k).cpu().numpy(), f"{tag} bisection against histogram, {k}", nonfinite=True)
    if order in ((0,), (0, "plain"), ("plain", 0)):
        close(res.I[:, n], ref["I"], f"{tag} I")
        close(res.Dn[:, n], ref["Dn"], f"{tag} Dn")


def bond_outputs(case, res, ref, kw, n=0):
    """(what, got, want) for every bond output the run wrote."""
    B = ref["B"]
    out = []
    if res.B_hist is not None:
        want = B[list(res.hist_epochs)]
        if res.B_hist.dtype == torch.bfloat16:
            want = torch.from_numpy(want.copy()).to(torch.bfloat16).float().numpy()  # round to nearest even
        out.append(("B_hist", res.B_hist[:, n], want))
    out.append(("B_final", res.B_final[n], B[-1]))
    if res.B_watch is not None:
        out.append(("B_watch", res.B_watch[:, n], B[list(res.hist_epochs)][:, :, list(res.watch_cols)]))
    if res.B_rows is not None:
        out.append(("B_rows", res.B_rows[:, n], B[list(res.hist_epochs)][:, list(res.watch_rows), :]))
    return out


def wn_case(case, part):
    clip = split_rows(case, part)
    for e in (0, 1, 2) if part == "all" else (0,):
        order = (e,)
        inp, W, S = tensors(case, "spread", order)
        ref, fam, tag = ref_of(case, "spread", order), fam_of(inp, order), f"{case.id} [{case.rank}] epoch {e}"
        res = engine.run(Y3, [params(Y3)], W, S, want=case.want)
        alt = engine.run(Y3, [params(Y3, nohist=True)], W, S, want=case.want)
        torch.cuda.synchronize()
        same(res.extra["Wn"][:, 0], ref["Wn"], f"{tag} Wn", fam, e == 2)
        same(res.extra["Wc"][0, 0], ref["Wc"], f"{tag} Wc", fam, e == 2, clip if e == 0 else None)
        if part == "mzero":
            return
        same(alt.extra["Wn"][:, 0], ref["Wn"], f"{tag} Wn (bisection run)", fam, e == 2)
        same(res.B_final[0], ref["B"][-1], f"{tag} B_final", fam, e == 2)
        check_common(case, res, alt, ref, order, tag)
        if e == 0:
            for k in ("R", "P"):
                if k in case.want:
                    close(res.extra[k][0, 0], ref[k], f"{tag} {k}")


def wn2_case(case, part):
    clip = split_rows(case, part)
    order = (0, "plain")
    inp, W, S = tensors(case, "spread", order)
    ref, fam, tag = ref_of(case, "spread", order), inp.family_of(0), f"{case.id} [{case.rank}]"
    res = engine.run(Y2, [params(Y2)], W, S, want=case.want)
    alt = engine.run(Y2, [params(Y2, nohist=True)], W, S, want=case.want)
    torch.cuda.synchronize()
    same(res.extra["Wn"][:, 0], ref["Wn"], f"{tag} Wn", fam)
    same(res.extra["Wc"][0, 0], ref["Wc"], f"{tag} Wc, epoch 0", fam, False, clip)
    from oracle import yuma_oracle as orc
    same(res.extra["Wc"][1, 0], orc.tmin(ref["Wn"][0], ref["C"][1][None, :]), f"{tag} Wc, epoch 1: the previous Wn", fam,
         False, clip)
    if part == "all":
        same(alt.extra["Wc"], res.extra["Wc"].cpu().numpy(), f"{tag} Wc, bisection against histogram")
        check_common(case, res, alt, ref, (0, "plain"), tag)


def bonds_case(case, part="all", stake="spread"):
    for order in ORDERS:
        inp, W, S = tensors(case, stake, order)
        E = len(order)
        kw = run_kw(case, inp, E)
        ref, fam = ref_of(case, stake, order), fam_of(inp, order)
        tag = f"{case.id} [{case.rank}, {case.scan}] epochs {order}"
        res = engine.run(case.variant, [params(case.variant)], W, S, want_hist=case.hist, want=case.want, **kw)
        alt = engine.run(case.variant, [params(case.variant, nohist=True)], W, S, want_hist=case.hist, want=case.want,
                         **kw) \
            if E == 1 else None
        torch.cuda.synchronize()
        for path in ("sched_path", "move_path", "rowstat_path", "resets_path", "watch_path", "rows_path"):
            assert res.extra.get(path, "native") == "native", f"{tag}: {path} {res.extra[path]}"
        if "hist_dtype" in kw:
            assert res.extra["hist_path"] == "bf16" and res.B_hist.dtype == torch.bfloat16
        for what, got, want in bond_outputs(case, res, ref, kw):
            same(got, want, f"{tag} {what}", fam, 2 in order)
        check_common(case, res, alt, ref, order, tag)
        if order == (0,) and "R" in case.want:
            close(res.extra["R"][0, 0], ref["R"], f"{tag} R")
        if order == (0,) and not kw:  # a two-scenario sweep of the same inputs against its replicated run
            prm = [params(case.variant), params(case.variant, nohist=True)]
            sw = engine.run(case.variant, prm, W, S, want_hist=case.hist, shared_inputs=True)
            rep = engine.run(case.variant, prm, W.expand(E, 2, case.V, case.M).contiguous(),
                             S.expand(E, 2, case.V).contiguous(), want_hist=case.hist)
            torch.cuda.synchronize()
            for k in ("C", "Dn", "I", "B_final"):
                same(getattr(sw, k), getattr(rep, k).cpu().numpy(), f"{tag} sweep against replicated, {k}")
            same(sw.B_final[0], ref["B"][-1], f"{tag} sweep B_final", fam)


def grp_case(case, part="all"):
    alphas = (0.5, 0.25, 0.5, 0.25)
    N = len(alphas)
    for order in ORDERS:
        inp, W, S = tensors(case, "spread", order)
        E, fam = len(order), fam_of(inp, order)
        tag = f"{case.id} [{case.rank}, {case.scan}] epochs {order}"
        prm = [params(Y4, a, nohist=(n == 3)) for n, a in enumerate(alphas)]
        sw = engine.run(Y4, prm, W, S, want_hist=case.hist, shared_inputs=True)
        rep = engine.run(Y4, prm, W.expand(E, N, case.V, case.M).contiguous(), S.expand(E, N, case.V).contiguous(),
                         want_hist=case.hist)
        torch.cuda.synchronize()
        for k in ("C", "Dn", "I", "B_final") + (("B_hist",) if case.hist else ()):
            same(getattr(sw, k), getattr(rep, k).cpu().numpy(), f"{tag} sweep against replicated, {k}", None, True)
        for n, a in enumerate(alphas):
            ref = ref_of(case, "spread", order, a)
            for what, got, want in bond_outputs(case, sw, ref, {}, n):
                same(got, want, f"{tag} scenario {n} (bond_alpha {a}) {what}", fam, 2 in order)
            check_common(case, sw, None, ref, order, f"{tag} scenario {n}", n)


def col_ties(case):
    """The stake pairs of the case whose run has a min(-0, +0) tie."""
    return [(n, i, j) for n, i, j in dc.pairs(case.V, case.M) if dc.tie_rows(case, ("pair", i, j))]


def col_case(case, part):
    variant = case.variant
    for name, i, j in dc.pairs(case.V, case.M) if part == "all" else col_ties(case):
        stake = ("pair", i, j)
        clip = split_rows(case, part, stake)
        inp, W, S = tensors(case, stake, (0,))
        ref, fam = ref_of(case, stake, (0,)), inp.family_of(0)
        tag = f"{case.id} [{case.scan}] stake on row {i} ({name}) and row {j} (plain)"
        res = engine.run(variant, [params(variant)], W, S, want_hist=case.hist, want=case.want)
        alt = engine.run(variant, [params(variant, nohist=True)], W, S, want_hist=case.hist, want=case.want)
        torch.cuda.synchronize()
        if case.hist:
            same(res.B_hist[0, 0], ref["B"][0], f"{tag} B_hist", fam, False, clip)
        same(res.B_final[0], ref["B"][0], f"{tag} B_final", fam, False, clip)
        for k, r in (("Wn", ref["Wn"][0]), ("Wb", ref.get("weight_for_bond")), ("B_inst", ref.get("validator_bond"))):
            if k in case.want:
                same(res.extra[k][0, 0], r, f"{tag} {k}", fam, False, None if k == "Wn" else clip)
        if part == "mzero":
            continue
        check_common(case, res, alt, ref, (0,), tag)


def y3pair_case(case, part="all"):
    inp0 = dc.build(case.V, case.M)
    stake = ("pair", inp0.rows["lo-out"][0], inp0.rows["plain"][3])
    bonds_case(case, part, stake)


KINDS = {"wn": wn_case, "wn2": wn2_case, "bonds": bonds_case, "grp": grp_case, "col": col_case, "y3pair": y3pair_case}


MIN_TIE = ("v_minimum3_f32 orders -0 below +0: W_c = min(Wn = -0, C = +0) is -0 (0x80000000) where torch and "
           "numpy return the second operand, +0; Yuma 0 / 1 / 2 carry the sign into a zero bond (DESIGN.md section 3)")


def items():
    out = []
    for c in dc.CASES:
        out.append(pytest.param(c, "all", id=c.id))
        if (c.kind in ("wn", "wn2") and dc.tie_rows(c)) or (c.kind == "col" and col_ties(c)):
            out.append(pytest.param(c, "mzero", id=c.id + "-mzero", marks=pytest.mark.xfail(strict=True, reason=MIN_TIE)))
    return out


@pytest.mark.parametrize("case,part", items())
def test_division_form_equals_ieee_division(case, part):
    KINDS[case.kind](case, part)


def test_uint16_weights_zero_row_and_full_row():
    """uint16 cannot hold the edge values: a zero row and a row of 65535s among
    plain integers, the native uint16 run against the widened run and the oracle."""
    V, M = 40, 132
    rng = np.random.default_rng(0xD171DE)
    W = rng.integers(0, 1000, (1, V, M)).astype(np.float32)
    W[0, 0] = 0
    W[0, V - 1] = 65535  # 132 * 65535 < 2^24: the row sum is exact
    S = dc.build(V, M).S[:1]
    dev = engine.device()
    Wd, Sd = torch.from_numpy(W[:, None].copy()).to(dev), torch.from_numpy(S[:, None].copy()).to(dev)
    from oracle import yuma_oracle as orc
    ref = orc.run(dc.VERSION[Y4], W, S, dc.Params(), return_weight=True)
    for hist in (True, False):
        u16 = engine.run(Y4, [params(Y4)], Wd.to(torch.uint16), Sd, want_hist=hist)
        f32 = engine.run(Y4, [params(Y4)], Wd, Sd, want_hist=hist)
        torch.cuda.synchronize()
        assert u16.extra["w_path"] == "u16" and f32.extra["w_path"] == "f32"
        for k in ("C", "Dn", "I", "B_final") + (("B_hist",) if hist else ()):
            same(getattr(u16, k), getattr(f32, k).cpu().numpy(), f"uint16 against widened, {k}")
        same(u16.B_final[0], ref["B"][0], "uint16 B_final against the oracle")
        same(u16.C[:, 0], ref["C"], "uint16 C against the oracle")
        assert np.array_equal(ref["B"][0], dc.yuma4_bits(dc.normalise(W[0])))
