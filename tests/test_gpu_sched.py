"""Input schedules (gpu marker): engine.run(..., sched=) over K stored slices
against engine.run on the expanded inputs W[sched], S[sched] at the same
options. Phase 1 is a pure function of one (W, S) slice, so every output must
have the dense run's bits: torch.equal on Dn, D, C, I, R, Sn, B_hist, B_final
(and bond_alpha, alpha_ab for liquid scenarios: the engine writes them for
those only), and extra["sched_path"] == "native".

Scan forms (plan_scan), named in the test ids:
  tile   (V=70, M=260, N=2) with history: k_bonds_elem R = 2 on 64-miner tiles
  wide   (V=12, M=1024, N=1) with history: the 512 x 1024 scan
  onerow both shapes without history: the one-row history-less form (DP_QTE)
  tworow (V=1024, M=4096, N=2) without history: N ceil(V/8) ceil(M/256) = 4096
         blocks, the threshold of the two-row history-less form; two stored
         slices of 32 MiB, five epochs
  bigv   (V=1100, M=64, N=1): the phase 1 above 1024 validators, the tile scan
E = 11 is a multiple of no ring depth (P = 2, 4)."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from conftest import assert_close
from oracle import yuma_oracle as orc

pytestmark = pytest.mark.gpu

from yuma_simulation._internal import engine, synth  # noqa: E402
from yuma_simulation._internal.cases import cases as builtin_cases  # noqa: E402
from yuma_simulation._internal.simulation_utils import SimulationRun, run_simulations  # noqa: E402
from yuma_simulation._internal.yumas import SimulationHyperparameters, YumaConfig, YumaParams  # noqa: E402

Y1, Y3, Y4 = engine.VARIANT_YUMA1, engine.VARIANT_YUMA3, engine.VARIANT_YUMA4
E = 11
SCHEDULES = {
    "identity": (11, list(range(11))),
    "constant": (1, [0] * 11),
    "alternating": (2, [0, 1] * 5 + [0]),
    "out-of-order": (3, [2, 2, 0, 0, 0, 1, 1, 2, 0, 1, 1]),
    "unreferenced": (4, [0, 1, 1, 2, 2, 2, 0, 0, 1, 2, 0]),  # slice 3 never read
}
OOO = SCHEDULES["out-of-order"]
SHAPES = {"tile": (2, 70, 260), "wide": (1, 12, 1024), "bigv": (1, 1100, 64), "tworow": (2, 1024, 4096)}
# the bond scan each (shape, history) of the tests below is there to reach under a schedule, as
# tests/test_scan_plan_host.py spells a plan (reached()); checked there without a GPU
REACH = {("tile", True): "tile_hist+sc", ("wide", True): "wide+sc", ("bigv", True): "tile_hist+sc",
         ("tile", False): "flat1+rq+sc", ("wide", False): "flat1+rq+sc", ("bigv", False): "flat1+rq+sc",
         ("tworow", False): "flat2+rq+sc"}
COVERED = {"wide", "tile_hist", "flat1", "flat2"}


def plan_args(shape, hist, variant):
    """engine.scan_plan's arguments for a native schedule run of SHAPES[shape]."""
    N, V, M = SHAPES[shape]
    return (variant, N, E, V, M), dict(want_hist=hist, sched=True)
VARIANTS = {"yuma3": (Y3, False), "yuma4": (Y4, False), "yuma4-liquid": (Y4, True)}
BASE = ("Dn", "C", "I", "B_final")
WANT = ("D", "R", "Sn")
LIQUID_WANT = ("bond_alpha", "alpha_ab")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "gpu tests need a ROCm GPU"
    engine.load_library()
    yield
    _INPUTS.clear()
    torch.cuda.empty_cache()


def config(liquid=False):
    return YumaConfig(simulation=SimulationHyperparameters(bond_penalty=0.99),
                      yuma_params=YumaParams(liquid_alpha=liquid))


_INPUTS: dict = {}


def stored(K, N, V, M, u16=False):
    """K stored slices on the device (built once per shape, never written)."""
    key = (K, N, V, M, u16)
    if key not in _INPUTS:
        seed = 0x5C4ED + 131 * V + M
        W = synth.weights(seed, K, N, V, M)
        S = synth.stakes(seed, K, N, V, period=1)
        if u16:
            assert (W == W.astype(np.uint16)).all()
            W = W.astype(np.uint16)
        _INPUTS[key] = (torch.from_numpy(W).cuda(), torch.from_numpy(S).cuda())
    return _INPUTS[key]


def take(t, sched):
    return engine._take_slices(t, torch.as_tensor(sched))


def outputs(res, liquid):
    names = WANT + (LIQUID_WANT if liquid else ())
    o = {"Dn": res.Dn, "C": res.C, "I": res.I, "B_final": res.B_final, **{k: res.extra[k] for k in names}}
    if res.B_hist is not None:
        o["B_hist"] = res.B_hist
    return o


def assert_same(got, ref, liquid, what=""):
    a, b = outputs(got, liquid), outputs(ref, liquid)
    assert a.keys() == b.keys()
    for k in a:
        x, y = engine._int_view(a[k]), engine._int_view(b[k])
        assert x.shape == y.shape and torch.equal(x, y), f"{what}: {k} differs"
    assert got.hist_epochs == ref.hist_epochs


def run_both(variant, params, W, S, sched, liquid, *, native=True, ref_kw=None, **kw):
    want = WANT + (LIQUID_WANT if liquid else ())
    kw.setdefault("want", want)
    ref = engine.run(variant, params, take(W, sched), take(S, sched), **{**kw, **(ref_kw or {})})
    got = engine.run(variant, params, W, S, sched=sched, **kw)
    assert got.extra["sched_path"] == ("native" if native else "expanded")
    assert "sched_path" not in ref.extra
    return got, ref


# ---------------------------------------------------------------------------
# schedules x scan forms x variants
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("vname", list(VARIANTS))
@pytest.mark.parametrize("shape", ["tile", "wide"])
@pytest.mark.parametrize("sname", list(SCHEDULES))
def test_schedules_with_history(sname, shape, vname):
    (K, sched), (N, V, M), (variant, liquid) = SCHEDULES[sname], SHAPES[shape], VARIANTS[vname]
    W, S = stored(K, N, V, M)
    params = [engine.make_params(variant, config(liquid))] * N
    got, ref = run_both(variant, params, W, S, sched, liquid, want_hist=True)
    assert_same(got, ref, liquid, f"{sname}-{shape}-{vname}")
    assert got.B_hist.shape == (E, N, V, M)


@pytest.mark.parametrize("vname", list(VARIANTS))
@pytest.mark.parametrize("shape", ["tile", "wide"])
@pytest.mark.parametrize("sname", ["alternating", "out-of-order"])
def test_schedules_without_history_onerow(sname, shape, vname):
    (K, sched), (N, V, M), (variant, liquid) = SCHEDULES[sname], SHAPES[shape], VARIANTS[vname]
    W, S = stored(K, N, V, M)
    params = [engine.make_params(variant, config(liquid))] * N
    got, ref = run_both(variant, params, W, S, sched, liquid)
    assert_same(got, ref, liquid)
    assert got.B_hist is None


@pytest.mark.parametrize("vname", ["yuma3", "yuma4-liquid"])
def test_without_history_tworow(vname):
    """The two-row history-less form starts at 4096 blocks of 8 rows x 256
    miners: N = 2, V = 1024, M = 4096 is the smallest grid that has them."""
    variant, liquid = VARIANTS[vname]
    (N, V, M), K = SHAPES["tworow"], 2
    assert N * ((V + 7) // 8) * ((M + 255) // 256) >= 4096
    key = ("tworow",)
    if key not in _INPUTS:
        W = engine.synth_weights(0x2205, K, N, V, M)
        S = torch.from_numpy(synth.stakes(0x2205, K, N, V, period=1)).cuda()
        _INPUTS[key] = (W, S)
    W, S = _INPUTS[key]
    sched = [1, 0, 0, 1, 0]
    params = [engine.make_params(variant, config(liquid))] * N
    got, ref = run_both(variant, params, W, S, sched, liquid, want=("D",) + (LIQUID_WANT if liquid else ()))
    for k in ("Dn", "C", "I", "B_final"):
        assert torch.equal(getattr(got, k), getattr(ref, k)), k
    assert torch.equal(got.extra["D"], ref.extra["D"])


@pytest.mark.parametrize("hist", [True, False], ids=["hist", "nohist"])
@pytest.mark.parametrize("vname", ["yuma3", "yuma4-liquid"])
def test_above_1024_validators_bigv(vname, hist):
    variant, liquid = VARIANTS[vname]
    (K, sched), (N, V, M) = OOO, SHAPES["bigv"]
    W, S = stored(K, N, V, M)
    params = [engine.make_params(variant, config(liquid))] * N
    got, ref = run_both(variant, params, W, S, sched, liquid, want_hist=hist)
    assert_same(got, ref, liquid)


# ---------------------------------------------------------------------------
# resets: reset_epoch is an epoch index; the conditional reset reads C[t - 1]
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["tile", "wide"])
def test_reset_always_inside_a_constant_segment(shape):
    (K, sched), (N, V, M) = OOO, SHAPES[shape]
    reset_epoch = 3  # sched[2:5] == [0, 0, 0]
    assert sched[reset_epoch - 1] == sched[reset_epoch] == sched[reset_epoch + 1]
    W, S = stored(K, N, V, M)
    params = [engine.make_params(Y3, config(), reset_mode=engine.RESET_ALWAYS, reset_epoch=reset_epoch,
                                 reset_index=M - 2, n_miners=M, n_epochs=E)] * N
    got, ref = run_both(Y3, params, W, S, sched, False, want_hist=True)
    assert_same(got, ref, False)
    # the reset happened, at the epoch and not at the slice's first use
    col = ref.B_hist[:, :, :, M - 2]
    assert bool((col[reset_epoch - 1] > 0).any())
    plain = engine.run(Y3, [engine.make_params(Y3, config())] * N, W, S, sched=sched, want_hist=True)
    assert not torch.equal(plain.B_hist[reset_epoch], got.B_hist[reset_epoch])
    assert torch.equal(plain.B_hist[:reset_epoch], got.B_hist[:reset_epoch])


@pytest.mark.parametrize("zero", [True, False], ids=["fires", "does-not-fire"])
@pytest.mark.parametrize("liquid", [False, True], ids=["scalar", "liquid"])
def test_reset_if_zero_consensus_reads_the_previous_epoch(zero, liquid):
    (K, sched), (N, V, M) = OOO, SHAPES["tile"]
    reset_epoch, idx = 5, 17  # sched[4] == 0, sched[5] == 1: the test reads slice 0's consensus
    assert sched[reset_epoch - 1] == 0 and sched[reset_epoch] == 1
    W, S = stored(K, N, V, M)
    W = W.clone()
    # slice 0: nobody weights the miner (its consensus is 0), or everybody at their row maximum
    W[0, :, :, idx] = 0.0 if zero else W[0].amax(dim=-1)
    params = [engine.make_params(Y4, config(liquid), reset_mode=engine.RESET_IF_ZERO_CONSENSUS,
                                 reset_epoch=reset_epoch, reset_index=idx, n_miners=M, n_epochs=E)] * N
    got, ref = run_both(Y4, params, W, S, sched, liquid, want_hist=True)
    assert_same(got, ref, liquid)
    c_prev = ref.C[reset_epoch - 1, :, idx]
    assert bool((c_prev == 0).all()) if zero else bool((c_prev > 0).all())
    plain = engine.run(Y4, [engine.make_params(Y4, config(liquid))] * N, W, S, sched=sched, want_hist=True)
    fired = not torch.equal(plain.B_hist[reset_epoch], got.B_hist[reset_epoch])
    assert fired == zero


# ---------------------------------------------------------------------------
# composition with the run's other options
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["tile", "wide"])
@pytest.mark.parametrize("vname", ["yuma3", "yuma4-liquid"])
def test_chunk_epochs_give_equal_bits(shape, vname):
    variant, liquid = VARIANTS[vname]
    (K, sched), (N, V, M) = OOO, SHAPES[shape]
    W, S = stored(K, N, V, M)
    params = [engine.make_params(variant, config(liquid))] * N
    want = WANT + (LIQUID_WANT if liquid else ())
    whole = engine.run(variant, params, W, S, sched=sched, want_hist=True, want=want, chunk_epochs=0)
    got, ref = run_both(variant, params, W, S, sched, liquid, want_hist=True, chunk_epochs=3)
    assert_same(got, ref, liquid)
    assert_same(got, whole, liquid)
    # ... and without the history (the one-row form parks its partials across chunks)
    a = engine.run(variant, params, W, S, sched=sched, want=want, chunk_epochs=0)
    b = engine.run(variant, params, W, S, sched=sched, want=want, chunk_epochs=3)
    assert_same(a, b, liquid)


COMPOSE = {
    "stride": dict(hist_stride=3, hist_first=1),
    "bf16": dict(hist_dtype=torch.bfloat16),
    "u16": dict(u16=True),
    "stride-bf16-u16": dict(hist_stride=3, hist_first=1, hist_dtype=torch.bfloat16, u16=True),
}


@pytest.mark.parametrize("shape", ["tile", "wide"])
@pytest.mark.parametrize("vname", ["yuma3", "yuma4-liquid"])
@pytest.mark.parametrize("cname", list(COMPOSE))
def test_composes_with_stride_bf16_and_uint16(cname, vname, shape):
    variant, liquid = VARIANTS[vname]
    kw = dict(COMPOSE[cname])
    u16 = kw.pop("u16", False)
    (K, sched), (N, V, M) = OOO, SHAPES[shape]
    W, S = stored(K, N, V, M, u16=u16)
    params = [engine.make_params(variant, config(liquid))] * N
    got, ref = run_both(variant, params, W, S, sched, liquid, want_hist=True, chunk_epochs=4, **kw)
    assert_same(got, ref, liquid, cname)
    assert got.extra["w_path"] == ref.extra["w_path"] == ("u16" if u16 else "f32")
    assert got.extra["hist_path"] == ref.extra["hist_path"] == ("bf16" if "hist_dtype" in kw else "f32")
    if "hist_stride" in kw:
        assert got.hist_epochs == (1, 4, 7, 10) and got.B_hist.shape[0] == 4
    if "hist_dtype" in kw:
        assert got.B_hist.dtype == torch.bfloat16


def test_uint16_without_history():
    (K, sched), (N, V, M) = OOO, SHAPES["tile"]
    W, S = stored(K, N, V, M, u16=True)
    params = [engine.make_params(Y4, config(True))] * N
    got, ref = run_both(Y4, params, W, S, sched, True)
    assert_same(got, ref, True)
    assert got.extra["w_path"] == "u16"


@pytest.mark.parametrize("shape", ["tile", "wide"])
@pytest.mark.parametrize("vname", ["yuma3", "yuma4-liquid"])
def test_resumed_and_split_runs(shape, vname):
    variant, liquid = VARIANTS[vname]
    (K, sched), (N, V, M) = OOO, SHAPES[shape]
    W, S = stored(K, N, V, M)
    params = [engine.make_params(variant, config(liquid))] * N
    whole, ref = run_both(variant, params, W, S, sched, liquid, want_hist=True)
    assert_same(whole, ref, liquid)
    # a resumed run: B_init supplied
    B0 = whole.B_hist[4].clone()
    got, ref2 = run_both(variant, params, W, S, sched, liquid, want_hist=True, B_init=B0)
    assert_same(got, ref2, liquid)
    # epochs [0, 6) then [6, 11) from B_final, each over the same stored slices
    first = engine.run(variant, params, W, S, sched=sched[:6], want_hist=True)
    second = engine.run(variant, params, W, S, sched=sched[6:], want_hist=True, B_init=first.B_final)
    assert first.extra["sched_path"] == second.extra["sched_path"] == "native"
    assert torch.equal(torch.cat([first.B_hist, second.B_hist]), whole.B_hist)
    assert torch.equal(torch.cat([first.Dn, second.Dn]), whole.Dn)
    assert torch.equal(torch.cat([first.C, second.C]), whole.C)
    assert torch.equal(torch.cat([first.I, second.I]), whole.I)
    assert torch.equal(second.B_final, whole.B_final)


# ---------------------------------------------------------------------------
# graphs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["tile", "wide"])
def test_graph_replays_and_follows_the_schedule_tensor(shape):
    (K, sched), (N, V, M) = OOO, SHAPES[shape]
    W, S = stored(K, N, V, M)
    params = [engine.make_params(Y4, config(True))] * N
    want = WANT + LIQUID_WANT
    direct = engine.run(Y4, params, W, S, sched=sched, want_hist=True, want=want)
    sd = torch.tensor(sched, dtype=torch.int32, device="cuda")
    g = engine.RunGraph(Y4, params, W, S, sched=sd, want_hist=True, want=want, chunk_epochs=4)
    try:
        assert g.result.extra["sched_path"] == "native" and g.result.extra["sched"] is sd
        assert g.nodes() > 0
        for _ in range(2):
            for t in outputs(g.result, True).values():
                t.fill_(float("nan"))
            res = g.launch()
            torch.cuda.synchronize()
            assert_same(res, direct, True, "replay")
        other = [1, 1, 2, 0, 0, 2, 2, 1, 0, 0, 1]
        sd.copy_(torch.tensor(other, dtype=torch.int32))
        res = g.launch()
        torch.cuda.synchronize()
        assert_same(res, engine.run(Y4, params, W, S, sched=other, want_hist=True, want=want), True, "rewritten")
    finally:
        g.close()


# ---------------------------------------------------------------------------
# fallbacks
# ---------------------------------------------------------------------------
def test_fallback_expands_outside_the_native_set():
    (K, sched), (N, V, M) = OOO, SHAPES["tile"]
    W, S = stored(K, N, V, M)
    p1 = [engine.make_params(Y1, config())] * N
    ref = engine.run(Y1, p1, take(W, sched), take(S, sched), want_hist=True)
    got = engine.run(Y1, p1, W, S, sched=sched, want_hist=True)
    assert got.extra["sched_path"] == "expanded" and got.extra["sched"] is None
    for k in ("Dn", "C", "I", "B_final", "B_hist"):
        assert torch.equal(getattr(got, k), getattr(ref, k)), k
    p3 = [engine.make_params(Y3, config())] * N
    ref = engine.run(Y3, p3, take(W, sched), take(S, sched), want=("Wn",))
    got = engine.run(Y3, p3, W, S, sched=sched, want=("Wn",))
    assert got.extra["sched_path"] == "expanded"
    assert torch.equal(got.extra["Wn"], ref.extra["Wn"]) and torch.equal(got.Dn, ref.Dn)
    assert torch.equal(got.B_final, ref.B_final)
    # miners not a multiple of 4: the scalar form
    W2, S2 = stored(K, 1, 70, 262)
    ref = engine.run(Y3, p3[:1], take(W2, sched), take(S2, sched))
    got = engine.run(Y3, p3[:1], W2, S2, sched=sched)
    assert got.extra["sched_path"] == "expanded" and torch.equal(got.Dn, ref.Dn)
    for bad in (dict(variant=Y1, params=p1), dict(variant=Y3, params=p3, want=("Wn",))):
        with pytest.raises(engine.EngineError, match="sched_native"):
            engine.RunGraph(bad.pop("variant"), bad.pop("params"), W, S, sched=sched, **bad)


def test_c_entry_point_refuses_yuma1_before_any_launch():
    lib = engine.load_library()
    (K, sched), (N, V, M) = OOO, SHAPES["tile"]
    W, S = stored(K, N, V, M)
    dev = W.device
    prm = engine.params_tensor([engine.make_params(Y1, config())] * N, dev)
    sd = torch.tensor(sched, dtype=torch.int32, device=dev)
    outs_t = {"Dn": torch.full((E, N, V), -7.0, device=dev), "C": torch.full((E, N, M), -7.0, device=dev),
              "I": torch.full((E, N, M), -7.0, device=dev), "B_final": torch.full((N, V, M), -7.0, device=dev)}
    outs = engine.YumaOutputsC(**{k: (outs_t[k].data_ptr() if k in outs_t else None) for k in engine.OUTPUT_FIELDS})
    nbytes = engine.workspace_bytes_sched(Y1, N, E, K, V, M, False)
    ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    args = (Y1, prm.data_ptr(), N, E, K, V, M, W.data_ptr(), S.data_ptr(), sd.data_ptr(), None, None,
            ctypes.addressof(outs), ws.data_ptr(), ws.numel(), 0, None)
    rc = lib.yuma_run_sched(*args, stream, None)
    assert rc == -4, rc  # YUMA_EUNSUPPORTED
    assert b"yuma_sched_native" in lib.yuma_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in outs_t.values())
    assert bool((ws == 0x5A).all())
    h = ctypes.c_void_p()
    assert lib.yuma_graph_create_sched(ctypes.byref(h), *args) == -4 and not h.value
    # bad arguments: YUMA_EINVAL, on a native variant too
    prm3 = engine.params_tensor([engine.make_params(Y3, config())] * N, dev)
    a3 = (Y3, prm3.data_ptr()) + args[2:]
    assert lib.yuma_run_sched(*a3[:4], 0, *a3[5:], stream, None) == -1  # K < 1
    assert lib.yuma_run_sched(*a3[:9], None, *a3[10:], stream, None) == -1  # NULL schedule
    bad = engine.YumaRunOptionsC(hist_stride=-1)
    assert lib.yuma_run_sched(*a3[:-1], ctypes.addressof(bad), stream, None) == -1
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in outs_t.values())


# ---------------------------------------------------------------------------
# oracle, and the simulation driver
# ---------------------------------------------------------------------------
def test_oracle_epoch_by_epoch_on_the_expanded_inputs():
    (K, sched), (N, V, M) = OOO, SHAPES["tile"]
    W, S = stored(K, N, V, M)
    cfg = config(True)
    got = engine.run(Y4, [engine.make_params(Y4, cfg)] * N, W, S, sched=sched, want_hist=True)
    assert got.extra["sched_path"] == "native"
    We, Se = W.cpu().numpy()[sched], S.cpu().numpy()[sched]
    for n in range(N):
        ref = orc.run("Yuma 4 (Rhef+relative bonds)", We[:, n], Se[:, n], cfg)
        np.testing.assert_array_equal(got.C[:, n].cpu().numpy(), ref["C"])
        assert_close(got.Dn[:, n].cpu().numpy(), ref["Dn"], what=f"Dn scenario {n}")
        assert_close(got.B_hist[:, n].cpu().numpy(), ref["B"], what=f"B scenario {n}")


def test_run_simulations_dedup_inputs():
    cfg = YumaConfig(simulation=SimulationHyperparameters(bond_penalty=0.99))
    liquid = YumaConfig(simulation=SimulationHyperparameters(bond_penalty=0.99),
                        yuma_params=YumaParams(liquid_alpha=True))
    picked = [builtin_cases[0], builtin_cases[3], builtin_cases[10]]
    for case in picked:
        Wp, Sp = case.packed_inputs()
        Wk, _, sched = engine.dedup_slices(Wp.unsqueeze(1), Sp.unsqueeze(1))
        assert Wk.shape[0] < Wp.shape[0] == sched.numel(), case.name
    runs = [SimulationRun(c, v, g) for c in picked
            for v, g in (("Yuma 3 (Rhef)", cfg), ("Yuma 1 (paper)", cfg), ("Yuma 4 (Rhef+relative bonds)", liquid))]
    base = run_simulations(runs)
    dedup = run_simulations(runs, dedup_inputs=True)
    for (d0, b0, i0), (d1, b1, i1) in zip(base, dedup):
        assert d0 == d1
        assert len(b0) == len(b1) and all(torch.equal(x, y) for x, y in zip(b0, b1))
        assert len(i0) == len(i1) and all(torch.equal(x, y) for x, y in zip(i0, i1))
