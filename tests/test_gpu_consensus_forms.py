"""Every kernel form of the consensus pass (gpu marker) on adversarial columns,
against an exact reference.

Inputs are tests/consensus_cases.py's: exact stakes, integer weights with
power-of-two row sums, column families built around kappa ties, grid ties,
zero-stake extremes, degenerate columns, mixed bracket widths, a column of
1.0, and an epoch with NaN / +-inf / negative / -0.0 entries. They are
order-independent, so C has to equal the big-integer reference
(consensus_cases.reference_C; tests/test_consensus_cases_host.py proves it
equal to the oracle and proves the families) bit for bit, on every column of
every epoch: no tie window, no masked column.

CASES names the kernel each shape is meant to reach (launch_consensus /
launch_consensus_mc in yuma_engine.hip choose by V, M % 4, the weight type,
shared inputs and a requested prerank P). Per case, over the 3 x 3 grid of
kappa in {0.3, 0.5, 0.7} and consensus_precision in {1000, 100000, 10000000}:

  * C of the two finite epochs, of the non-finite epoch and of the epoch with
    a column above 1.0 equals the reference;
  * on the finite epochs Dn, I and B_final agree with oracle.run within the
    suite's RTOL / ATOL_FRAC (conftest, unchanged);
  * the histogram run and the YUMA_FLAG_NO_HIST run are bit-equal;
  * a shared-input sweep equals its replicated run bit for bit, the sharded C
    concatenated equals the unsharded C.

make_params accepts kappa = 0.0 and kappa = 1.0 (it checks no range, as the
reference checks none); they run on the `extra_kappas` cases. kappa = 1.0 is
what reaches `lo_c > 0 && !(stot > kappa)`: the stakes total exactly 1."""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import pytest
import torch

import consensus_cases as cc
from conftest import ATOL_FRAC, RTOL, assert_close
from oracle import yuma_oracle as orc

pytestmark = pytest.mark.gpu

from yuma_simulation._internal import engine, wide  # noqa: E402
from yuma_simulation._internal.yumas import SimulationHyperparameters, YumaConfig  # noqa: E402

RUST, Y3 = engine.VARIANT_RUST, engine.VARIANT_YUMA3
VERSION = {RUST: "Yuma 0 (subtensor)", Y3: "Yuma 3 (Rhef)"}
GRID = tuple((k, p) for k in cc.KAPPAS for p in cc.PRECISIONS)
EDGE_KAPPAS = ((0.0, 100000), (1.0, 100000), (1.0, 1000), (0.0, 10000000))


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "gpu tests need a ROCm GPU"
    engine.load_library()
    yield
    torch.cuda.empty_cache()


@dataclass(frozen=True)
class Case:
    id: str
    kernel: str               # the form the shape is meant to reach
    V: int
    M: int
    stake: str
    kind: str = "run"         # run | P | sweep | u16 | shards
    variant: int = Y3
    extra_kappas: bool = False


CASES = [
    Case("w1", "k_consensus_w<1, true>", 13, 36, "u24"),
    Case("w1-rows16", "k_consensus_w<1, true>, no padding rows", 16, 36, "u20", extra_kappas=True),
    Case("w4", "k_consensus_w<4, true>", 40, 132, "u20"),
    Case("w4-yuma0", "k_consensus_w<4, true>, fp64 consensus", 40, 132, "u20", variant=RUST),
    Case("w4-rows64", "k_consensus_w<4, true>, no padding rows", 64, 132, "u24", extra_kappas=True),
    Case("p-V70", "k_consensus_p<true>", 70, 260, "u24"),
    Case("p-V70-yuma0", "k_consensus_p<true>, fp64 consensus", 70, 260, "u24", variant=RUST),
    Case("p-V200", "k_consensus_p<true>", 200, 132, "u20"),
    Case("p-rows256", "k_consensus_p<true>, no padding rows", 256, 260, "u20", extra_kappas=True),
    Case("p-single", "k_consensus_p<true>, one validator holds all the stake", 70, 260, "single"),
    Case("w16-scalar", "k_consensus_w<16, false>", 70, 262, "u20"),
    Case("w16-P", "k_consensus_w<16, true> (prerank requested)", 70, 260, "u24", kind="P"),
    Case("block-vector", "k_consensus<1024, 16, true>", 300, 68, "u24", extra_kappas=True),
    Case("block-scalar", "k_consensus<1024, 16, false>", 300, 67, "u20"),
    Case("block-single", "k_consensus<1024, 16, true>, one validator holds all the stake", 300, 68, "single"),
    Case("big", "k_consensus_big<true>", 1100, 96, "u20"),
    Case("mc1", "k_consensus_mc<1, true>", 13, 36, "u24", kind="sweep"),
    Case("mc4", "k_consensus_mc<4, true>", 40, 132, "u20", kind="sweep"),
    Case("mc16", "k_consensus_mc<16, true>", 70, 260, "u24", kind="sweep"),
    Case("u16-w1", "k_consensus_w<1, true, uint16_t>", 13, 36, "u24", kind="u16"),
    Case("u16-w4", "k_consensus_w<4, true, uint16_t>", 40, 132, "u20", kind="u16"),
    Case("u16-p", "k_consensus_p<true, uint16_t>", 70, 260, "u24", kind="u16"),
    Case("u16-block", "k_consensus<1024, 16, true, uint16_t>", 300, 68, "u24", kind="u16"),
    Case("shards", "the shard-stage launch_consensus (k_consensus_p, 2 shards)", 130, 520, "u24", kind="shards"),
]


# validators per form (row_cfg, launch_consensus: 16 / 64 / 256 / YUMA_REG_VALIDATORS)
RANGES = (("k_consensus_w<1,", (1, 16)), ("k_consensus_w<4,", (17, 64)), ("k_consensus_w<16,", (65, 256)),
          ("k_consensus_p<", (65, 256)), ("k_consensus<1024, 16,", (257, 1024)), ("k_consensus_big<", (1025, 1 << 20)),
          ("k_consensus_mc<1,", (1, 16)), ("k_consensus_mc<4,", (17, 64)), ("k_consensus_mc<16,", (65, 256)),
          ("the shard-stage launch_consensus (k_consensus_p", (65, 256)))


def test_case_table_matches_the_dispatch():
    """The shapes sit where the table says: validator ranges of row_cfg /
    launch_consensus, vector forms at M % 4 == 0, and the input builder knows
    every shape (so the host test has proved its conditions)."""
    for c in CASES:
        assert (c.V, c.M, c.stake) in cc.SHAPES, c.id
        lo, hi = next(r for prefix, r in RANGES if c.kernel.startswith(prefix))
        assert lo <= c.V <= hi, c.id
        assert (c.M % 4 == 0) == ("false>" not in c.kernel), c.id
        assert c.kind != "u16" or c.M % 4 == 0


def config(kappa, precision):
    return YumaConfig(simulation=SimulationHyperparameters(kappa=kappa, consensus_precision=precision))


def params(variant, kappa, precision, nohist=False):
    p = engine.make_params(variant, config(kappa, precision))
    if nohist:
        p.flags |= engine.FLAG_NO_HIST
    return p


_ORACLE: dict = {}


def oracle_run(case, kappa, precision):
    """oracle.run over the two finite epochs (computed once per shape and setting)."""
    key = (case.V, case.M, case.stake, case.variant, kappa, precision)
    if key not in _ORACLE:
        inp = cc.build(case.V, case.M, case.stake)
        _ORACLE[key] = orc.run(VERSION[case.variant], inp.W[:2], inp.S[:2], config(kappa, precision))
    return _ORACLE[key]


def check_close(actual, expected, what):
    a, e = np.asarray(actual, np.float64), np.asarray(expected, np.float64)
    if a.shape == e.shape and np.isfinite(e).all() and np.isfinite(a).all() and e.size:
        tol = ATOL_FRAC * np.abs(e).max() + RTOL * np.abs(e)
        err = np.abs(a - e)
        ratio = float(np.max(np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))))
        print(f"[consensus forms] {what}: worst error / tolerance = {ratio:.4f}")
    assert_close(actual, expected, what=what)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(x, y, tag):
    for k in ("C", "Dn", "I", "B_final"):
        assert torch.equal(bits(getattr(x, k)), bits(getattr(y, k))), f"{tag}: {k} differs"


def check_C(got, ref, inp, tag):
    """Bit-equal C [E, M]; a mismatch names the columns and their families."""
    got = got.cpu().numpy()
    if not np.array_equal(got, ref):
        fam = {c: n for n, cols in inp.columns.items() for c in cols}
        bad = [(int(e), int(m), fam.get(int(m), "-"), float(got[e, m]), float(ref[e, m]))
               for e, m in zip(*np.nonzero(got != ref))]
        raise AssertionError(f"{tag}: C differs from the exact reference at (epoch, column, family, got, want) "
                             f"{bad[:12]} ({len(bad)} in all)")


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_consensus_form_equals_exact_reference(case):
    dev = engine.device()
    V, M, variant = case.V, case.M, case.variant
    inp = cc.build(V, M, case.stake)
    dbl = variant == RUST
    Wd = torch.from_numpy(inp.W[:, None].copy()).to(dev)   # [4, 1, V, M] (the cached inputs stay read-only)
    Sd = torch.from_numpy(inp.S[:, None].copy()).to(dev)
    if case.kind == "u16":
        assert inp.W[:2].max() <= 65535 and (inp.W[:2] == np.floor(inp.W[:2])).all()
        W16 = torch.from_numpy(inp.W[:2, None].astype(np.uint16)).to(dev)
    want = ("P",) if case.kind == "P" else ()
    grid = GRID + (EDGE_KAPPAS if case.extra_kappas else ())

    if case.kind == "sweep":
        return sweep(case, inp, Wd, Sd, dev)

    for kappa, precision in grid:
        tag = f"{case.id} [{case.kernel}] kappa {kappa} precision {precision}"
        ref = cc.reference_C(V, M, case.stake, kappa, precision, dbl)
        runs = {}
        for nohist in (False, True):
            prm = [params(variant, kappa, precision, nohist)]
            if case.kind == "u16":
                fin = engine.run(variant, prm, W16, Sd[:2])
                assert fin.extra["w_path"] == "u16", tag
                odd = None  # (uint16 holds no NaN, inf or negative weight)
            else:
                fin = engine.run(variant, prm, Wd[:2], Sd[:2], want=want)
                odd = engine.run(variant, prm, Wd[2:], Sd[2:], want=want)
                assert fin.extra["w_path"] == "f32"
            torch.cuda.synchronize()
            runs[nohist] = (fin, odd)
            which = "bisection" if nohist else "histogram"
            check_C(fin.C[:, 0], ref[:2], inp, f"{tag} {which}, finite epochs")
            if odd is not None:
                check_C(odd.C[:, 0], ref[2:], inp, f"{tag} {which}, non-finite and above-one epochs")
        same_bits(runs[False][0], runs[True][0], f"{tag} histogram against bisection")
        if runs[False][1] is not None:
            assert torch.equal(runs[False][1].C, runs[True][1].C), f"{tag} histogram against bisection, odd epochs"
        fin = runs[False][0]
        o = oracle_run(case, kappa, precision)
        np.testing.assert_array_equal(o["C"], ref[:2])
        check_close(fin.Dn[:, 0].cpu().numpy(), o["Dn"], f"{tag} Dn")
        check_close(fin.I[:, 0].cpu().numpy(), o["I"], f"{tag} I")
        check_close(fin.B_final[0].cpu().numpy(), o["B"][-1], f"{tag} B_final")
        if case.kind == "P":  # prerank (yumas.py:192): the wave-owned kernel's own sum
            Wn, Sn = cc.normalise(inp.W[:2]).astype(np.float64), np.stack([cc.normalise_stake(s) for s in inp.S[:2]])
            check_close(fin.extra["P"][:, 0].cpu().numpy(), np.einsum("ev,evm->em", Sn.astype(np.float64), Wn),
                        f"{tag} P")
        if case.kind == "shards":
            prm = [params(variant, kappa, precision)]
            for W, S, r, whole in ((Wd[:2], Sd[:2], ref[:2], runs[False][0]), (Wd[2:], Sd[2:], ref[2:], runs[False][1])):
                ws = wide.run_wide_local(variant, prm, W, S, 2)
                torch.cuda.synchronize()
                assert len(ws.C) == 2 and all(c.shape[2] < M for c in ws.C)
                C = torch.cat(ws.C, dim=2)
                check_C(C[:, 0], r, inp, f"{tag} sharded")
                assert torch.equal(C, whole.C), f"{tag}: sharded C differs from the unsharded"


def sweep(case, inp, Wd, Sd, dev):
    """Six scenarios on shared inputs in four consensus classes (kappa,
    precision, YUMA_FLAG_NO_HIST); scenarios 0 and 3 share one. Then every
    flag flipped: each scenario's histogram run against its bisection run."""
    V, M, variant = case.V, case.M, case.variant
    settings = [(0.5, 100000, False), (0.3, 1000, False), (0.7, 10000000, True),
                (0.5, 100000, False), (0.3, 10000000, True), (0.7, 1000, False)]
    more = [(0.7, 100000, True), (0.5, 1000, True), (0.3, 100000, False),
            (0.7, 100000, True), (0.5, 10000000, False), (0.5, 10000000, True)]
    N = len(settings)
    for sets in (settings, more):
        assert len({s for s in sets}) >= 3 and len({s for s in sets}) < N
        got = {}
        for flip in (False, True):
            prm = [params(variant, k, p, nh != flip) for k, p, nh in sets]
            for name, sl in (("finite", slice(0, 2)), ("odd", slice(2, 4))):
                E = 2
                sw = engine.run(variant, prm, Wd[sl], Sd[sl], shared_inputs=True)
                rep = engine.run(variant, prm, Wd[sl].expand(E, N, V, M).contiguous(),
                                 Sd[sl].expand(E, N, V).contiguous())
                torch.cuda.synchronize()
                assert sw.C.shape == (E, N, M)
                tag = f"{case.id} [{case.kernel}] {name} epochs"
                assert torch.equal(sw.C, rep.C), f"{tag}: sweep C differs from the replicated run"
                if name == "finite":
                    same_bits(sw, rep, f"{tag} sweep against replicated")
                for n, (k, p, _) in enumerate(sets):
                    ref = cc.reference_C(V, M, case.stake, k, p, False)
                    check_C(sw.C[:, n], ref[sl], inp, f"{tag} scenario {n} kappa {k} precision {p}")
                got[flip, name] = sw
        same_bits(got[False, "finite"], got[True, "finite"], f"{case.id} histogram against bisection")
        assert torch.equal(got[False, "odd"].C, got[True, "odd"].C)
        fin = got[False, "finite"]
        for n, (k, p, _) in enumerate(sets):
            o = oracle_run(case, k, p)
            tag = f"{case.id} scenario {n}"
            check_close(fin.Dn[:, n].cpu().numpy(), o["Dn"], f"{tag} Dn")
            check_close(fin.I[:, n].cpu().numpy(), o["I"], f"{tag} I")
            check_close(fin.B_final[n].cpu().numpy(), o["B"][-1], f"{tag} B_final")
