"""Resumed runs (gpu marker): a caller's bond state B_init [N,V,M] and, for
Yuma 2, previous normalised weights Wprev_init [N,V,M] on every bond scan and
rank form of the multi-epoch run (engine.run, engine.RunGraph,
wide.run_wide_local).

For each launch shape of plan_scan / launch_rank (CASES names the kernel a
shape is meant to reach):

  * bitwise split: run(E) == run(E1) followed by run(E - E1, B_init = B_final
    of the first segment, Wprev_init = Wn[E1 - 1]) in Dn, C, I, B_hist, B_final
    -- Bstate and B_init enter a scan by the same load;
  * oracle from a foreign state: four epochs from a B0 / Wp0 the recurrence
    cannot reach (above the Yuma 3 cap, above 1 for Yuma 4, an all-zero and a
    one-hot column for the column-normalised variants, an all-zero row,
    distinct per scenario) against oracle.run(..., B_init=, W_prev_init=):
    C exact, the rest within the suite's tolerance (conftest RTOL, ATOL_FRAC).

Inputs are synth.weights / synth.stakes(period=3): consensus is exact, every
element is compared. E = 11, E1 = 5: the split falls inside a turn of every
in-flight ring (1..4 epochs) and the second segment wraps each of them."""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import pytest
import torch

from conftest import ATOL_FRAC, RTOL, assert_close
from oracle import yuma_oracle as orc

pytestmark = pytest.mark.gpu

from yuma_simulation._internal import engine, synth, wide  # noqa: E402
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
E, E1, E4 = 11, 5, 4


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
    hist: bool
    liquid: bool = False
    kind: str = "run"        # run | offset | sweep | u16 | graph | shards
    reset: str | None = None  # "always" (at whole-run epoch E1) | "if_zero_c" (at E1 + 1)
    scenarios: tuple = ()     # the scenarios compared with the oracle (default: all)
    device_inputs: bool = False
    # the bond scan the case is there to reach, as tests/test_scan_plan_host.py spells a plan (reached()):
    # kernel or k_bonds_elem shape, then +rq +hs +bf16 +sc +u16 and /scalar; checked there without a GPU
    reach: str = ""


def _cases():
    c = []
    # k_bonds RC_256_1 / RC_256_4 (column-normalised, <= 64 validators), the
    # 64-miner-tile history scan for Yuma 3 / 4; Yuma 2: k_rank_s without column sums
    for V, rows in ((16, 1), (40, 4)):
        c += [Case(f"small{V}-{NAME[v]}", v, 2, V, 132, True,
                   reach="tile_hist" if v in (Y3, Y4) else f"k_bonds<256,{rows}>") for v in ALL5]
    # k_bonds_cn at 1, 2, 4, 8 rows per lane, a half-filled last strip (72 = 4 * 16 + 8)
    c += [Case(f"strip-V{V}", RUST, 2, V, 72, True, reach=f"k_bonds_cn<{rows}>+rq")
          for V, rows in ((100, 1), (200, 2), (384, 4), (1000, 8))]
    # k_bonds_elem 512 x 1024 (Yuma 1 / 2 on the screened reciprocal, Yuma 3 / 4
    # without), second column block 4 miners wide; Yuma 2: k_rank_sw with column sums
    c += [Case(f"widehist-{NAME[v]}", v, 2, 70, 1028, True, liquid=v == Y4, reach="wide+rq" if v in (Y1, Y2) else "wide")
          for v in (Y1, Y2, Y3, Y4)]
    # k_bonds_elem R = 2 on 64-miner tiles (DP_TV)
    c += [Case(f"tilehist-{NAME[v]}", v, 2, 70, 260, True, reach="tile_hist") for v in (Y1, Y2, Y3, Y4)]
    # the one-row history-less scan, epoch-minor partials + k_dte_sum
    c += [Case(f"nohist1-{NAME[v]}", v, 2, 70, 260, False, liquid=v == Y4, reach="flat1+rq") for v in (Y1, Y2, Y3, Y4)]
    # the two-row history-less scan: blocks_r2 = 32 * 8 * 16 = 4096 (Yuma 3; Yuma 1
    # at 64 validators forms no column sums and takes k_bonds RC_256_4 on 2048
    # blocks, so a 72-validator Yuma 1 case, 29 * 9 * 16 = 4176, reaches the scan)
    c += [Case("nohist2-yuma3", Y3, 32, 64, 4096, False, scenarios=(0, 17, 31), device_inputs=True, reach="flat2+rq"),
          Case("nohist2-yuma1", Y1, 32, 64, 4096, False, scenarios=(0, 17, 31), device_inputs=True,
               reach="k_bonds<256,4>"),
          Case("nohist2-yuma1-V72", Y1, 29, 72, 4096, False, scenarios=(0, 28), device_inputs=True, reach="flat2+rq")]
    # the VEC = false forms (M % 4 != 0)
    for hist in (True, False):
        c += [Case(f"scalar-{'hist' if hist else 'nohist'}-{NAME[v]}", v, 1, 70, 262, hist,
                   reach="k_bonds<256,16>/scalar" if v == RUST else "flat1/scalar") for v in ALL5]
    # B_init 4 bytes into a larger buffer: the run drops to the scalar kernels
    c += [Case(f"offset-{NAME[v]}", v, 1, 70, 260, True, kind="offset",
               reach="k_bonds<256,16>/scalar" if v == RUST else "flat1/scalar") for v in (Y3, RUST)]
    # k_bonds_grp: one full group of 4 scenarios and one of 2, per-scenario B_init
    for hist in (True, False):
        c += [Case(f"sweep-{'hist' if hist else 'nohist'}-{NAME[v]}", v, 6, 70, 260, hist, kind="sweep",
                   reach="k_bonds_grp+rq+hist" if hist else "k_bonds_grp+rq") for v in (Y3, Y4)]
    # k_rust_big_ema / k_rust_big_norm, the element-wise scan above 1024
    # validators, the big k_rank_sw with Wprev_init
    c += [Case(f"bigv-{NAME[v]}", v, 1, 1100, 96, True, reach="k_rust_big" if v == RUST else "tile_hist")
          for v in (RUST, Y1, Y2, Y3)]
    # native uint16 W with an fp32 B_init
    c += [Case("u16-yuma3", Y3, 2, 70, 1028, True, kind="u16", reach="wide+u16"),
          Case("u16-yuma4-liquid", Y4, 2, 70, 260, False, liquid=True, kind="u16", reach="flat1+rq+u16")]
    # the reset on the caller's state at epoch 0 / at epoch 1 of the second segment
    c += [Case(f"reset0-{NAME[v]}", v, 2, 70, 1028, True, reset="always", reach="wide") for v in (Y3, Y4)]
    c += [Case("reset1-yuma3", Y3, 2, 70, 260, False, reset="if_zero_c", reach="flat1+rq")]
    c += [Case(f"graph-{NAME[v]}", v, 2, 64, 512, True, kind="graph", reach="tile_hist" if v == Y3 else "k_bonds<256,4>")
          for v in (Y3, Y2)]
    # the shard stages, three shards of 192, 192 and 136 columns (no screened reciprocals there: k_bonds_cn
    # without RQ for Yuma 0; Yuma 2 forms its column sums in a stage too and takes the element-wise scan)
    c += [Case(f"shards-{NAME[v]}", v, 1, 130, 520, True, kind="shards",
               reach="k_bonds_cn<2>" if v == RUST else "tile_hist") for v in (RUST, Y2, Y3)]
    return c


def plan_args(case, shard=None):
    """engine.scan_plan's arguments for the scan a case's runs launch. The
    shards cases: stage 4 of the first column shard, and (shard=False) the
    plain run they are compared with."""
    shard = case.kind == "shards" if shard is None else shard
    M = len(wide.column_ranges(case.M, 3)[0]) if shard else case.M
    return (case.variant, case.N, E, case.V, M), dict(
        want_hist=case.hist, shared_inputs=case.kind == "sweep", w_u16=case.kind == "u16",
        vector_form=M % 4 == 0 and case.kind != "offset", shard_stage=shard)


# what the plain runs of the shards cases reach (520 miners, with the screened reciprocals)
SHARDS_RUN_REACH = {"shards-rust": "k_bonds_cn<2>+rq", "shards-yuma2": "tile_hist", "shards-yuma3": "tile_hist"}


# every (kernel or shape, strip rows) the list reaches: a case taken out or moved must leave this as it is
COVERED = {"k_bonds<256,1>", "k_bonds<256,4>", "k_bonds<256,16>", "k_bonds_cn<1>", "k_bonds_cn<2>", "k_bonds_cn<4>",
           "k_bonds_cn<8>", "k_rust_big", "k_bonds_grp", "wide", "tile_hist", "flat1", "flat2"}


CASES = _cases()


def reset_column(M):
    return M - 2  # in the last, partly filled column block of every shape used


def configs(case):
    """One configuration per scenario. The sweep mixes fixed and liquid alpha
    and two kappas over its six scenarios, and gives each its own bond_alpha,
    decay_rate and capacity_alpha: Yuma 3's bonds depend on the last two only
    (yumas.py:452-476), and with equal bonds in every scenario the split could
    not tell one scenario's state from another's. Every other case shares one."""
    if case.kind == "sweep":
        return [YumaConfig(simulation=SimulationHyperparameters(kappa=0.45 + 0.1 * (i % 2), bond_penalty=0.99),
                           yuma_params=YumaParams(bond_alpha=0.05 + 0.04 * i, liquid_alpha=i % 3 == 1,
                                                  decay_rate=0.1 + 0.02 * i, capacity_alpha=0.1 + 0.01 * i))
                for i in range(case.N)]
    cfg = YumaConfig(simulation=SimulationHyperparameters(bond_penalty=0.99),
                     yuma_params=YumaParams(liquid_alpha=case.liquid))
    return [cfg] * case.N


def make_params(case, cfgs, reset_epoch, n_epochs, resumed):
    kw = {}
    if case.reset is not None:
        mode = engine.RESET_ALWAYS if case.reset == "always" else engine.RESET_IF_ZERO_CONSENSUS
        kw = dict(reset_mode=mode, reset_epoch=reset_epoch, reset_index=reset_column(case.M),
                  n_miners=case.M, n_epochs=n_epochs, resumed=resumed)
    return [engine.make_params(case.variant, c, **kw) for c in cfgs]


def inputs(case, dev):
    """W [E,Nw,V,M], S [E,Nw,V] on the device (Nw = 1 for the sweep) and the
    CPU copies of the scenarios the oracle reads, {n: (W [E4+,V,M], S)}."""
    Nw = 1 if case.kind == "sweep" else case.N
    seed = 0x2E5 + 131 * case.V + case.M + case.variant
    col = reset_column(case.M)
    S = synth.stakes(seed, E, Nw, case.V, period=3)
    if case.device_inputs:  # the large shapes: the device twin of synth.weights (bit-identical)
        Wd = engine.synth_weights(seed, E, Nw, case.V, case.M)
    else:
        W = synth.weights(seed, E, Nw, case.V, case.M)
        if case.reset == "if_zero_c":
            # zero consensus on the reset column at whole-run epoch E1 (segment
            # epoch 0) and at epoch 0 (the foreign-state run resets at its epoch 1)
            W[E1, :, :, col] = 0.0
            W[0, :, :, col] = 0.0
        Wd = torch.from_numpy(W).to(dev)
    scen = case.scenarios or tuple(range(case.N))
    host = {}
    for n in scen:
        nw = 0 if Nw == 1 else n
        host[n] = (Wd[:E4, nw].cpu().numpy(), S[:E4, nw])
    return Wd, torch.from_numpy(S).to(dev), host


def normalised(W):
    """The oracle's fp32 W / (rowsum + 1e-6) (yumas.py:186-187)."""
    rs = W.sum(axis=-1, dtype=np.float32)
    return (W / (rs + np.float32(1e-6))[..., None]).astype(np.float32)


def foreign_state(case, S0, rng):
    """B0 [N,V,M] no run produces, and Wp0 [N,V,M] (row-normalised, unrelated
    to any W). S0 [N,V]: the raw stakes of the first epoch."""
    N, V, M = case.N, case.V, case.M
    u = rng.random((N, V, M), dtype=np.float32)
    if case.variant == Y3:  # up to 1.5 x the cap S_n * 2^64: both clamps act
        Sn = (S0 / S0.sum(axis=1, dtype=np.float32)[:, None]).astype(np.float32)
        cap = (Sn * np.float32(float(2**64 - 1))).astype(np.float32)
        B0 = (u * np.float32(1.5) * cap[:, :, None]).astype(np.float32)
        assert (B0 > cap[:, :, None]).any()
    elif case.variant == Y4:
        B0 = (u * np.float32(1.25)).astype(np.float32)
        assert (B0 > 1).any()
    else:  # columns summing to 1 over the validators, one all-zero, one one-hot
        B0 = (u / u.sum(axis=1, dtype=np.float32)[:, None, :]).astype(np.float32)
        B0[:, :, 3] = 0.0
        B0[:, :, M - 1] = 0.0
        B0[:, V // 2, M - 1] = 1.0
    B0[:, V - 3, :] = 0.0  # one all-zero row
    w = rng.random((N, V, M), dtype=np.float32)
    Wp0 = (w / w.sum(axis=2, dtype=np.float32)[:, :, None]).astype(np.float32)
    return B0, Wp0


def check_close(actual, expected, what):
    """assert_close at the suite's defaults; prints the worst error as a
    fraction of the tolerance first (pytest -s)."""
    a = np.asarray(actual, np.float64)
    e = np.asarray(expected, np.float64)
    if a.shape == e.shape and np.isfinite(e).all() and np.isfinite(a).all() and e.size:
        tol = ATOL_FRAC * np.abs(e).max() + RTOL * np.abs(e)
        err = np.abs(a - e)
        ratio = float(np.max(np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))))
        print(f"[resume] {what}: worst error / tolerance = {ratio:.4f}")
    assert_close(actual, expected, what=what)


def check_oracle(res, n, ref, hist, tag):
    np.testing.assert_array_equal(res.C[:, n].cpu().numpy(), ref["C"], err_msg=f"{tag} C")
    check_close(res.Dn[:, n].cpu().numpy(), ref["Dn"], f"{tag} Dn")
    check_close(res.I[:, n].cpu().numpy(), ref["I"], f"{tag} I")
    if hist:
        check_close(res.B_hist[:, n].cpu().numpy(), ref["B"], f"{tag} B_hist")
    check_close(res.B_final[n].cpu().numpy(), ref["B"][-1], f"{tag} B_final")


def assert_same_bits(x, y, hist, tag, lo=0):
    """x == y[lo:] in the per-epoch outputs, and the final state."""
    for k in ("Dn", "C", "I") + (("B_hist",) if hist else ()):
        assert torch.equal(getattr(x, k), getattr(y, k)[lo:]), f"{tag}: {k} differs"
    assert torch.equal(x.B_final, y.B_final), f"{tag}: B_final differs"


def gathered(w: wide.WideResult, hist) -> engine.RunResult:
    """A sharded result with its column blocks joined."""
    return engine.RunResult(w.Dn, torch.cat(w.C, dim=2), torch.cat(w.I, dim=2), torch.cat(w.B_final, dim=2),
                            torch.cat(w.B_hist, dim=3) if hist else None, {})


def oracle_from(case, cfg, Wh, Sh, B0, Wp0, reset_epoch):
    """oracle.run over the host inputs of one scenario from (B0, Wp0)."""
    version, kw = VERSION[case.variant], {}
    col = reset_column(case.M)
    if case.reset == "always" and reset_epoch == 0:
        if case.variant == Y3:
            version, kw = "Yuma 3.1 (Rhef+reset)", dict(reset_epoch=0, reset_index=col)
        else:  # (no Yuma 4 version resets always: state it as the zeroed column of the state)
            B0 = B0.copy()
            B0[:, col] = 0.0
    elif case.reset == "if_zero_c":
        version, kw = "Yuma 3.2 (Rhef+conditional)", dict(reset_epoch=reset_epoch, reset_index=col)
    return orc.run(version, Wh, Sh, cfg, B_init=B0, W_prev_init=Wp0, **kw)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_resumed_run_equals_whole_run_and_oracle(case):
    dev = engine.device()
    variant, N, hist = case.variant, case.N, case.hist
    cfgs = configs(case)
    Wd, Sd, host = inputs(case, dev)
    shared = case.kind == "sweep"
    if case.kind == "u16":
        Wf, Wh = Wd, Wd.cpu().numpy()
        assert (Wh == Wh.astype(np.uint16)).all()  # synth weights are integers below 2^16 at these widths
        Wd = torch.from_numpy(Wh.astype(np.uint16)).to(dev)

    def run(W, S, params, B=None, Wp=None):
        return engine.run(variant, params, W, S, B, Wp, want_hist=hist, shared_inputs=shared)

    # whole-run reset epochs: "always" at E1 (segment epoch 0), conditional at E1 + 1 (segment epoch 1)
    r_whole = {None: None, "always": E1, "if_zero_c": E1 + 1}[case.reset]
    r_seg = None if r_whole is None else r_whole - E1
    p_whole = make_params(case, cfgs, r_whole, E, False)
    p_a = make_params(case, cfgs, r_whole, E1, False)
    p_b = make_params(case, cfgs, r_seg, E - E1, True)

    # --- Yuma 2: the previous epoch's normalised weights that seed segment 2
    Wn = None
    if variant == Y2:
        Wn = torch.from_numpy(normalised(Wd[E1 - 1].cpu().numpy())).to(dev)
        own = engine.run(variant, p_a, Wd[E1 - 1:E1], Sd[E1 - 1:E1], want=("Wn",))
        assert torch.equal(own.extra["Wn"][0], Wn), "the engine's W_n is not the oracle's fp32 W / (rowsum + 1e-6)"

    # --- the bitwise split
    if case.kind != "offset":
        whole = run(Wd, Sd, p_whole)
        a = run(Wd[:E1], Sd[:E1], p_a)
        b = run(Wd[E1:], Sd[E1:], p_b, a.B_final, Wn)
        torch.cuda.synchronize()
        if case.kind == "u16":
            assert whole.extra["w_path"] == a.extra["w_path"] == b.extra["w_path"] == "u16"
            bf = run(Wf[E1:], Sd[E1:], p_b, a.B_final, Wn)
            assert bf.extra["w_path"] == "f32"
            assert_same_bits(b, bf, hist, f"{case.id} uint16 against fp32")
        assert_same_bits(b, whole, hist, f"{case.id} resumed against whole", lo=E1)
        if case.reset == "always":  # the reset fired on the caller's state at segment epoch 0
            plain = run(Wd[E1:], Sd[E1:], make_params(case, cfgs, None, E - E1, True), a.B_final, Wn)
            col = reset_column(case.M)
            assert not torch.equal(plain.B_hist[0, :, :, col], b.B_hist[0, :, :, col])
        if case.reset == "if_zero_c":  # ... at segment epoch 1, on the zero consensus of epoch 0
            plain = run(Wd[E1:], Sd[E1:], make_params(case, cfgs, None, E - E1, True), a.B_final, Wn)
            col = reset_column(case.M)
            assert bool((b.C[0, :, col] == 0).all())
            assert not torch.equal(plain.B_final[:, :, col], b.B_final[:, :, col])
        if shared:  # the sweep against the replicated run, from the same per-scenario state
            V, M = case.V, case.M
            rep = engine.run(variant, p_b, Wd[E1:].expand(E - E1, N, V, M).contiguous(),
                             Sd[E1:].expand(E - E1, N, V).contiguous(), a.B_final, want_hist=hist)
            assert_same_bits(b, rep, hist, f"{case.id} sweep against replicated")
        if case.kind == "shards":
            ws = wide.run_wide_local(variant, p_b, Wd[E1:], Sd[E1:], 3, B_init=a.B_final, Wprev_init=Wn,
                                     want_hist=hist)
            torch.cuda.synchronize()
            g = gathered(ws, hist)
            # as tests/test_wide.py for a fresh run: consensus and the
            # column-local bonds bitwise, the cross-shard sums within tolerance
            for k in ("C", "B_hist", "B_final"):
                assert torch.equal(getattr(g, k), getattr(b, k)), f"{case.id}: sharded {k} differs"
            check_close(g.I.cpu().numpy(), b.I.cpu().numpy(), f"{case.id} sharded I")
            check_close(g.Dn.cpu().numpy(), b.Dn.cpu().numpy(), f"{case.id} sharded Dn")
        if case.kind == "graph":
            Bc, Wc = a.B_final.clone(), None if Wn is None else Wn.clone()
            graph = engine.RunGraph(variant, p_b, Wd[E1:], Sd[E1:], Bc, Wc, want_hist=hist)
            assert graph.result.extra["_inputs"][2].data_ptr() == Bc.data_ptr()  # captured in place
            r = graph.launch()
            torch.cuda.synchronize()
            assert_same_bits(r, b, hist, f"{case.id} graph replay")

    # --- the oracle, from a foreign state
    rng = np.random.default_rng(0xB0 + case.V + case.M)
    B0, Wp0 = foreign_state(case, Sd[0].expand(N, case.V).cpu().numpy() if shared else Sd[0].cpu().numpy(), rng)
    if variant != Y2:
        Wp0 = None
    B0d = torch.from_numpy(B0).to(dev)
    Wp0d = None if Wp0 is None else torch.from_numpy(Wp0).to(dev)
    if case.kind == "offset":
        buf = torch.empty(B0d.numel() + 4, dtype=torch.float32, device=dev)
        view = buf[1:1 + B0d.numel()].view(B0d.shape)
        view.copy_(B0d)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        B0d = view
    r_f = {None: None, "always": 0, "if_zero_c": 1}[case.reset]
    p_f = make_params(case, cfgs, r_f, E4, True)
    c = run(Wd[:E4], Sd[:E4], p_f, B0d, Wp0d)
    torch.cuda.synchronize()
    if case.kind == "offset":
        assert c.extra["_inputs"][2].data_ptr() == view.data_ptr()
    if case.kind == "u16":
        assert c.extra["w_path"] == "u16"
    refs = {}
    for n, (Wh, Sh) in host.items():
        refs[n] = oracle_from(case, cfgs[n], Wh, Sh, B0[n], None if Wp0 is None else Wp0[n], r_f)
        check_oracle(c, n, refs[n], hist, f"{case.id} scenario {n}")
    if case.reset == "if_zero_c":  # the conditional reset fired at epoch 1 of the foreign run too
        ref0 = orc.run(VERSION[variant], *host[0], cfgs[0], B_init=B0[0])
        col = reset_column(case.M)
        assert refs[0]["C"][0, col] == 0.0
        assert not np.array_equal(ref0["B"][1][:, col], refs[0]["B"][1][:, col])
    if case.kind == "shards":
        ws = wide.run_wide_local(variant, p_f, Wd[:E4], Sd[:E4], 3, B_init=B0d, Wprev_init=Wp0d, want_hist=hist)
        torch.cuda.synchronize()
        check_oracle(gathered(ws, hist), 0, refs[0], hist, f"{case.id} sharded")
    if case.kind == "graph":
        # refill both captured states in place, replay: a direct run from them
        Bc.copy_(B0d)
        if Wc is not None:
            Wc.copy_(Wp0d)
        r = graph.launch()
        torch.cuda.synchronize()
        direct = run(Wd[E1:], Sd[E1:], p_b, B0d, Wp0d)
        torch.cuda.synchronize()
        assert_same_bits(r, direct, hist, f"{case.id} graph replay after refill")
        assert not torch.equal(direct.B_final, b.B_final)
        graph.close()


@pytest.mark.parametrize("variant", [Y1, Y3, Y4], ids=lambda v: NAME[v])
def test_zero_state_and_no_state(variant):
    """B_init = zeros against no B_init at the tilehist shape: the same bits
    for Yuma 3 / Yuma 4 (their update from nothing is the update from zero
    bonds, yumas.py:452, :570); another run for Yuma 1, whose EMA applies from
    epoch 0 once a state exists (yumas.py:254-258) -- checked on the oracle."""
    case = Case(f"zeros-{NAME[variant]}", variant, 2, 70, 260, True)
    dev = engine.device()
    cfgs = configs(case)
    Wd, Sd, host = inputs(case, dev)
    params = make_params(case, cfgs, None, E4, False)
    zeros = torch.zeros(case.N, case.V, case.M, device=dev)
    z = engine.run(variant, params, Wd[:E4], Sd[:E4], zeros, want_hist=True)
    none = engine.run(variant, params, Wd[:E4], Sd[:E4], want_hist=True)
    torch.cuda.synchronize()
    if variant in (Y3, Y4):
        for k in ("Dn", "I", "B_hist"):
            assert torch.equal(getattr(z, k), getattr(none, k)), f"{NAME[variant]}: {k} from zeros differs"
    else:
        assert not torch.equal(z.B_hist[0], none.B_hist[0])
        for n, (Wh, Sh) in host.items():
            ref = orc.run(VERSION[variant], Wh, Sh, cfgs[n], B_init=np.zeros((case.V, case.M), np.float32))
            check_oracle(z, n, ref, True, f"yuma1 from zeros scenario {n}")


@pytest.mark.parametrize("name", ["B_init", "Wprev_init"])
@pytest.mark.parametrize("shape", ["VM", "wider", "more_scenarios"])
def test_wrong_shaped_state_is_refused(name, shape):
    """A state that is not [N,V,M] raises ValueError before anything is
    launched (a [V,M] tensor for N = 2 would be read past its end)."""
    N, V, M = 2, 8, 128
    dev = engine.device()
    W = torch.ones(2, N, V, M, device=dev)
    S = torch.ones(2, N, V, device=dev)
    good = torch.zeros(N, V, M, device=dev)
    bad = torch.zeros({"VM": (V, M), "wider": (N, V, M + 4), "more_scenarios": (N + 1, V, M)}[shape], device=dev)
    params = [engine.make_params(Y2, YumaConfig())] * N
    kw = {"B_init": good, "Wprev_init": good, name: bad}
    out = {k: torch.full(s, -7.0, device=dev)
           for k, s in (("Dn", (2, N, V)), ("C", (2, N, M)), ("I", (2, N, M)), ("B_final", (N, V, M)))}
    with pytest.raises(ValueError, match=name):
        engine.run(Y2, params, W, S, kw["B_init"], kw["Wprev_init"], out=out)
    with pytest.raises(ValueError, match=name):
        engine.RunGraph(Y2, params, W, S, kw["B_init"], kw["Wprev_init"], out=out)
    with pytest.raises(ValueError, match=name):
        wide.run_wide_local(Y2, params, W, S, 2, **kw)
    # the shard path itself, one tensor per shard
    cols = wide.column_ranges(M, 2)
    sh = {k: [t[..., c.start:c.stop] if t.dim() == 3 else t for c in cols] for k, t in kw.items()}
    if shape == "wider":  # the extra columns land in the last shard
        sh[name][-1] = bad[..., cols[-1].start:]
    with pytest.raises(ValueError, match=name):
        wide._run_shards(Y2, params, [W[..., c.start:c.stop] for c in cols], S, cols, M,
                         lambda xs, widths=None: xs, cols, **sh)
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in out.values())  # nothing was launched
