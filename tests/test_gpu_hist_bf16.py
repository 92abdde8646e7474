"""bfloat16 bond history (gpu marker): engine.run(..., hist_dtype=torch.bfloat16)
on the two scans that write it natively (k_bonds_elem in its wide and its
64-miner-tile shape, Yuma 3 / Yuma 4, fp32 and uint16 weights, dense and
strided, direct and as a graph) and on the fallbacks that convert an fp32
history.

  * bitwise: B_hist, read as int16, is the fp32-history run's B_hist converted
    to bfloat16 on the CPU (round to nearest even), at the stored epochs; the
    fp32 history holds no NaN, and some element of every case rounds up, so a
    truncating store fails;
  * Dn, C, I and B_final have the fp32-history run's bits;
  * no stray or over-wide stores: the history sits between two guard slices
    holding a bfloat16 NaN pattern, which a store of fp32 width or at fp32
    offsets would overwrite; a history of no slots writes nothing;
  * the oracle at every epoch, within a bfloat16 half-ulp (2^-9) with a factor
    2 of margin on top of the suite's fp32 tolerance;
  * the fallbacks say "f32" and return the same bits; RunGraph refuses them;
    the C entry point refuses the flag outside the native set before any launch;
  * run_simulations(..., bonds_dtype=torch.bfloat16).

Inputs are those of tests/test_gpu_hist_stride.py: synth.weights /
synth.stakes(period=3), E = 11, chunk_epochs = 4, bond_penalty = 0.99."""

from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np
import pytest
import torch

from conftest import ATOL_FRAC, RTOL, assert_close
from oracle import yuma_oracle as orc

pytestmark = pytest.mark.gpu

from yuma_simulation._internal import engine, synth  # noqa: E402
from yuma_simulation._internal.cases import cases as builtin_cases  # noqa: E402
from yuma_simulation._internal.simulation_utils import SimulationRun, run_simulations  # noqa: E402
from yuma_simulation._internal.yumas import (  # noqa: E402
    SimulationHyperparameters,
    YumaConfig,
    YumaParams,
)

RUST, Y1, Y3, Y4 = engine.VARIANT_RUST, engine.VARIANT_YUMA1, engine.VARIANT_YUMA3, engine.VARIANT_YUMA4
NAME = {RUST: "rust", Y1: "yuma1", Y3: "yuma3", Y4: "yuma4"}
VERSION = {RUST: "Yuma 0 (subtensor)", Y1: "Yuma 1 (paper)", Y3: "Yuma 3 (Rhef)", Y4: "Yuma 4 (Rhef+relative bonds)"}
E = 11
CHUNK = 4  # chunks [0,4) [4,8) [8,11): stored epochs on both sides of a boundary, chunks with t0 != 0
STRIDES = ((3, None), (5, 7))  # (stride, first): first None = stride - 1
RESET_EPOCH = 5
GUARD = 0x7FDE  # a bfloat16 NaN's bits, as int16
BF16 = torch.bfloat16
# a bfloat16 half-ulp is 2^-9 relative; a factor 2 of margin, on top of the fp32 tolerance
ORACLE_RTOL = 2.0 ** -8 + RTOL


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "gpu tests need a ROCm GPU"
    engine.load_library()
    yield
    _FP32.clear()
    torch.cuda.empty_cache()


@dataclass(frozen=True)
class Case:
    id: str
    variant: int
    N: int
    V: int
    M: int
    liquid: bool = False
    kind: str = "run"  # run | sweep | u16 | graph
    reset: bool = False  # Yuma 3, reset_mode ALWAYS at RESET_EPOCH
    strided: bool = False  # also run under STRIDES
    # the bond scan the case is there to reach with a dense bfloat16 history, as tests/test_scan_plan_host.py
    # spells a plan (reached()); checked there without a GPU. FALLBACK cases are refused a native history.
    reach: str = ""


NATIVE = [
    # k_bonds_elem 512 x 1024, second column block 4 miners wide
    Case("wide-yuma3", Y3, 2, 70, 1028, strided=True, reach="wide+bf16"),
    Case("wide-yuma4-liquid", Y4, 2, 70, 1028, liquid=True, strided=True, reach="wide+bf16"),
    # k_bonds_elem R = 2 on 64-miner tiles
    Case("tile-yuma3", Y3, 2, 70, 260, strided=True, reach="tile_hist+bf16"),
    Case("tile-yuma4", Y4, 2, 70, 260, strided=True, reach="tile_hist+bf16"),
    # one and two row blocks' worth of validators below a full block, a half-filled last tile
    Case("small16-yuma3", Y3, 2, 16, 132, reach="tile_hist+bf16"), Case("small16-yuma4", Y4, 2, 16, 132, reach="tile_hist+bf16"),
    Case("small40-yuma3", Y3, 2, 40, 132, reach="tile_hist+bf16"), Case("small40-yuma4", Y4, 2, 40, 132, reach="tile_hist+bf16"),
    # the same kernel above 1024 validators
    Case("bigv-yuma3", Y3, 1, 1100, 96, reach="tile_hist+bf16"),
    Case("u16-yuma3", Y3, 2, 70, 1028, kind="u16", reach="wide+bf16+u16"),
    Case("reset-wide-yuma3", Y3, 2, 70, 1028, reset=True, reach="wide+bf16"),
    Case("reset-tile-yuma3", Y3, 2, 70, 260, reset=True, reach="tile_hist+bf16"),
    Case("graph-yuma3", Y3, 2, 64, 512, kind="graph", reach="tile_hist+bf16"),
]
FALLBACK = [
    Case("yuma1", Y1, 2, 70, 260),
    Case("rust", RUST, 2, 100, 72),
    Case("scalar-yuma3", Y3, 1, 70, 262),
    Case("sweep-yuma3", Y3, 6, 70, 260, kind="sweep"),
]


def plan_args(case, strided=False):
    """engine.scan_plan's arguments for a case's native bfloat16 runs (strided: stride 3 from epoch 2)."""
    return (case.variant, case.N, E, case.V, case.M), dict(
        want_hist=True, hist_bf16=True, hist_stride=3 if strided else 1, shared_inputs=case.kind == "sweep",
        w_u16=case.kind == "u16")


# every k_bonds_elem shape the native list reaches, dense and (strided cases) with +hs
COVERED = {"wide", "tile_hist"}


def configs(case):
    if case.kind == "sweep":  # as tests/test_gpu_hist_stride.py: no two scenarios hold the same bonds
        return [YumaConfig(simulation=SimulationHyperparameters(kappa=0.45 + 0.1 * (i % 2), bond_penalty=0.99),
                           yuma_params=YumaParams(bond_alpha=0.05 + 0.04 * i, liquid_alpha=i % 3 == 1,
                                                  decay_rate=0.1 + 0.02 * i, capacity_alpha=0.1 + 0.01 * i))
                for i in range(case.N)]
    cfg = YumaConfig(simulation=SimulationHyperparameters(bond_penalty=0.99),
                     yuma_params=YumaParams(liquid_alpha=case.liquid))
    return [cfg] * case.N


def make_params(case, cfgs):
    kw = {}
    if case.reset:
        kw = dict(reset_mode=engine.RESET_ALWAYS, reset_epoch=RESET_EPOCH, reset_index=case.M - 2,
                  n_miners=case.M, n_epochs=E)
    return [engine.make_params(case.variant, c, **kw) for c in cfgs]


def inputs(case, dev):
    Nw = 1 if case.kind == "sweep" else case.N
    seed = 0x57D + 131 * case.V + case.M + case.variant
    W = synth.weights(seed, E, Nw, case.V, case.M)
    S = synth.stakes(seed, E, Nw, case.V, period=3)
    if case.kind == "u16":
        assert (W == W.astype(np.uint16)).all()
        Wd = torch.from_numpy(W.astype(np.uint16)).to(dev)
    else:
        Wd = torch.from_numpy(W).to(dev)
    return W, S, Wd, torch.from_numpy(S).to(dev)


def run_kw(case):
    return dict(chunk_epochs=CHUNK, shared_inputs=case.kind == "sweep")


_FP32: dict = {}  # per case: everything the fp32-history run gives, computed once and left unchanged


def fp32_run(case):
    """(params, W host, S host, W dev, S dev, the fp32-history run, its history
    as bfloat16 bits converted on the CPU, its history as truncated bits)."""
    if case.id not in _FP32:
        dev = engine.device()
        params = make_params(case, configs(case))
        W, S, Wd, Sd = inputs(case, dev)
        ref = engine.run(case.variant, params, Wd, Sd, want_hist=True, **run_kw(case))
        torch.cuda.synchronize()
        hist = ref.B_hist.cpu()
        assert ref.B_hist.dtype == torch.float32 and ref.extra["hist_path"] == "f32"
        assert not bool(torch.isnan(hist).any()), f"{case.id}: the fp32 history holds a NaN"
        rne = hist.to(BF16).view(torch.int16)  # the CPU's conversion: round to nearest even
        trunc = (hist.view(torch.int32) >> 16).to(torch.int16)
        _FP32[case.id] = (params, W, S, Wd, Sd, ref, rne, trunc)
    return _FP32[case.id]


def guarded(slots, case, dev):
    """A bfloat16 history of `slots` slices between two guard slices."""
    buf = torch.full((slots + 2, case.N, case.V, case.M), GUARD, dtype=torch.int16, device=dev).view(BF16)
    return buf, buf[1:1 + slots]


def assert_guards(buf, tag):
    raw = buf.view(torch.int16)
    for g in (0, -1):
        assert bool((raw[g] == GUARD).all()), f"{tag}: a store outside the history"


def assert_bf16_of(res, case, epochs, tag, path):
    """res is the bfloat16-history run of `case` at `epochs`."""
    _, _, _, _, _, ref, rne, trunc = fp32_run(case)
    assert res.extra["hist_path"] == path, f"{tag}: hist_path {res.extra['hist_path']}"
    assert res.B_hist.dtype == BF16 and res.hist_epochs == tuple(epochs), tag
    assert tuple(res.B_hist.shape) == (len(epochs), case.N, case.V, case.M), tag
    got = res.B_hist.cpu().view(torch.int16)
    idx = list(epochs)
    assert torch.equal(got, rne[idx]), f"{tag}: B_hist is not RNE(fp32 history)"
    if idx:  # rounding is exercised: plain truncation gives other bits somewhere
        assert bool((rne[idx] != trunc[idx]).any()), f"{tag}: no element rounds up, truncation would pass"
    for k in ("Dn", "C", "I", "B_final"):
        assert torch.equal(getattr(res, k), getattr(ref, k)), f"{tag}: {k} differs from the fp32-history run"


@pytest.mark.parametrize("case", NATIVE, ids=[c.id for c in NATIVE])
def test_native_history_is_the_rounded_fp32_history(case):
    dev = engine.device()
    params, _, _, Wd, Sd, ref, _, _ = fp32_run(case)
    assert engine.hist_bf16_native(case.variant, case.N, E, case.V, case.M)
    if case.kind == "u16":
        assert ref.extra["w_path"] == "u16"
    if case.reset:  # the reset acts on the stored state
        col = ref.B_hist[:, :, :, case.M - 2]
        assert bool((col[RESET_EPOCH - 1] != 0).any()) and bool((col[RESET_EPOCH + 1] != col[RESET_EPOCH - 1]).any())

    # dense, between guards
    buf, hist = guarded(E, case, dev)
    res = engine.run(case.variant, params, Wd, Sd, hist_dtype=BF16, out={"B_hist": hist}, **run_kw(case))
    torch.cuda.synchronize()
    assert res.B_hist.data_ptr() == hist.data_ptr()
    if case.kind == "u16":
        assert res.extra["w_path"] == "u16"
    assert_bf16_of(res, case, range(E), f"{case.id} dense", "bf16")
    assert_guards(buf, f"{case.id} dense")

    # dense, the engine's own allocation, one chunk
    res = engine.run(case.variant, params, Wd, Sd, want_hist=True, hist_dtype=BF16)
    torch.cuda.synchronize()
    assert_bf16_of(res, case, range(E), f"{case.id} dense, one chunk", "bf16")

    if case.strided:
        for stride, first in STRIDES:
            epochs = engine.hist_epochs(E, stride, first)
            tag = f"{case.id} stride {stride} first {first}"
            buf, hist = guarded(len(epochs), case, dev)
            res = engine.run(case.variant, params, Wd, Sd, hist_dtype=BF16, hist_stride=stride, hist_first=first,
                             out={"B_hist": hist}, **run_kw(case))
            torch.cuda.synchronize()
            assert_bf16_of(res, case, epochs, tag, "bf16")
            assert_guards(buf, tag)

    # a history of no slots (first = E) writes nothing
    buf, hist = guarded(0, case, dev)
    res = engine.run(case.variant, params, Wd, Sd, hist_dtype=BF16, hist_stride=2, hist_first=E,
                     out={"B_hist": hist}, **run_kw(case))
    torch.cuda.synchronize()
    assert res.hist_epochs == () and res.B_hist.shape[0] == 0 and res.B_hist.dtype == BF16
    assert_guards(buf, f"{case.id} no slots")
    for k in ("Dn", "C", "I", "B_final"):
        assert torch.equal(getattr(res, k), getattr(ref, k)), f"{case.id} no slots: {k} differs"

    if case.kind == "graph":
        graph = engine.RunGraph(case.variant, params, Wd, Sd, want_hist=True, hist_dtype=BF16, chunk_epochs=CHUNK)
        for replay in range(2):
            graph.result.B_hist.view(torch.int16).fill_(GUARD)
            r = graph.launch()
            torch.cuda.synchronize()
            assert_bf16_of(r, case, range(E), f"{case.id} graph replay {replay}", "bf16")
        graph.close()
        graph = engine.RunGraph(case.variant, params, Wd, Sd, want_hist=True, hist_dtype=BF16, hist_stride=3,
                                chunk_epochs=CHUNK)
        r = graph.launch()
        torch.cuda.synchronize()
        assert_bf16_of(r, case, engine.hist_epochs(E, 3), f"{case.id} strided graph", "bf16")
        graph.close()


def test_eight_byte_aligned_history_is_native_and_an_odd_one_falls_back():
    """B_hist needs 8-byte alignment only; a view at 2 bytes past it cannot
    take 8-byte stores, so the run converts an fp32 history into it."""
    case = NATIVE[2]
    dev = engine.device()
    params, _, _, Wd, Sd, _, _, _ = fp32_run(case)
    n = E * case.N * case.V * case.M
    for off, path in ((4, "bf16"), (1, "f32")):
        flat = torch.full((n + 16,), GUARD, dtype=torch.int16, device=dev).view(BF16)
        hist = flat[off:off + n].view(E, case.N, case.V, case.M)
        assert hist.data_ptr() % 16 == 2 * off
        res = engine.run(case.variant, params, Wd, Sd, hist_dtype=BF16, out={"B_hist": hist}, **run_kw(case))
        torch.cuda.synchronize()
        assert res.B_hist.data_ptr() == hist.data_ptr()
        assert_bf16_of(res, case, range(E), f"offset {off}", path)
        raw = flat.view(torch.int16)
        assert bool((raw[:off] == GUARD).all()) and bool((raw[off + n:] == GUARD).all())


ORACLE_CASES = [NATIVE[2], Case("tile-yuma4-liquid", Y4, 2, 70, 260, liquid=True), NATIVE[0]]


@pytest.mark.parametrize("case", ORACLE_CASES, ids=[c.id for c in ORACLE_CASES])
def test_stored_epochs_match_the_oracle(case):
    params, W, S, Wd, Sd, _, _, _ = fp32_run(case)
    cfgs = configs(case)
    res = engine.run(case.variant, params, Wd, Sd, want_hist=True, hist_dtype=BF16, **run_kw(case))
    torch.cuda.synchronize()
    assert res.extra["hist_path"] == "bf16"
    hist = res.B_hist.cpu().to(torch.float32).numpy()
    for n in range(case.N):
        ref = orc.run(VERSION[case.variant], W[:, n], S[:, n], cfgs[n])
        np.testing.assert_array_equal(res.C[:, n].cpu().numpy(), ref["C"], err_msg=f"{case.id} C")
        for t in range(E):
            assert_close(hist[t, n], ref["B"][t], rtol=ORACLE_RTOL, atol_frac=ATOL_FRAC,
                         what=f"{case.id} scenario {n} B[{t}]")


@pytest.mark.parametrize("case", FALLBACK, ids=[c.id for c in FALLBACK])
def test_fallbacks_convert_an_fp32_history_and_say_so(case):
    dev = engine.device()
    params, _, _, Wd, Sd, _, _, _ = fp32_run(case)
    assert not engine.hist_bf16_native(case.variant, case.N, E, case.V, case.M, shared_inputs=case.kind == "sweep")
    res = engine.run(case.variant, params, Wd, Sd, want_hist=True, hist_dtype=BF16, **run_kw(case))
    torch.cuda.synchronize()
    assert_bf16_of(res, case, range(E), case.id, "f32")
    # into the caller's buffer, strided
    epochs = engine.hist_epochs(E, 3)
    buf, hist = guarded(len(epochs), case, dev)
    res = engine.run(case.variant, params, Wd, Sd, hist_dtype=BF16, hist_stride=3, out={"B_hist": hist},
                     **run_kw(case))
    torch.cuda.synchronize()
    assert res.B_hist.data_ptr() == hist.data_ptr()
    assert_bf16_of(res, case, epochs, f"{case.id} stride 3", "f32")
    assert_guards(buf, case.id)


def test_run_graph_refuses_the_fallback():
    case = FALLBACK[0]
    params, _, _, Wd, Sd, _, _, _ = fp32_run(case)
    with pytest.raises(engine.EngineError, match="hist_bf16_native"):
        engine.RunGraph(case.variant, params, Wd, Sd, want_hist=True, hist_dtype=BF16, chunk_epochs=CHUNK)


def test_bad_history_buffers_raise():
    case = NATIVE[4]
    dev = engine.device()
    params, _, _, Wd, Sd, _, _, _ = fp32_run(case)
    shape = (E, case.N, case.V, case.M)
    with pytest.raises(ValueError, match="bfloat16"):  # an fp32 buffer for a bfloat16 history
        engine.run(case.variant, params, Wd, Sd, hist_dtype=BF16, out={"B_hist": torch.empty(shape, device=dev)})
    with pytest.raises(ValueError, match="B_hist"):  # the wrong slot count
        engine.run(case.variant, params, Wd, Sd, hist_dtype=BF16, hist_stride=3,
                   out={"B_hist": torch.empty(shape, dtype=BF16, device=dev)})
    with pytest.raises(ValueError, match="hist_dtype"):
        engine.run(case.variant, params, Wd, Sd, want_hist=True, hist_dtype=torch.float16)
    # torch.float32 is today's path
    res = engine.run(case.variant, params, Wd, Sd, want_hist=True, hist_dtype=torch.float32, **run_kw(case))
    torch.cuda.synchronize()
    assert res.B_hist.dtype == torch.float32 and torch.equal(res.B_hist, fp32_run(case)[5].B_hist)


def _c_call(variant, N, V, M, flags, with_hist):
    """yuma_run_opts with every pointer valid and sized for an fp32 history, so
    that the call could only write in bounds; the outputs hold a sentinel."""
    dev = engine.device()
    lib = engine.load_library()
    Ec = 2
    W = torch.ones((Ec, N, V, M), dtype=torch.float32, device=dev)
    S = torch.ones((Ec, N, V), dtype=torch.float32, device=dev)
    cfg = YumaConfig(simulation=SimulationHyperparameters(bond_penalty=0.99))
    prm = engine.params_tensor([engine.make_params(variant, cfg)] * N, dev)
    shapes = [("Dn", (Ec, N, V)), ("C", (Ec, N, M)), ("I", (Ec, N, M)), ("B_final", (N, V, M))]
    if with_hist:
        shapes.append(("B_hist", (Ec, N, V, M)))
    o = {k: torch.full(s, -7.0, dtype=torch.float32, device=dev) for k, s in shapes}
    outs = engine.YumaOutputsC(**{k: (o[k].data_ptr() if k in o else None) for k in engine.OUTPUT_FIELDS})
    ws = torch.empty(engine.workspace_bytes(variant, N, Ec, V, M, False), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    opts = engine.YumaRunOptionsC(flags=flags)
    rc = lib.yuma_run_opts(variant, prm.data_ptr(), N, Ec, V, M, W.data_ptr(), S.data_ptr(), None, None,
                           ctypes.addressof(outs), ws.data_ptr(), ws.numel(), 0, ctypes.addressof(opts), stream, None)
    err = lib.yuma_last_error()
    h = ctypes.c_void_p()
    rcg = lib.yuma_graph_create_opts(ctypes.byref(h), variant, prm.data_ptr(), N, Ec, V, M, W.data_ptr(),
                                     S.data_ptr(), None, None, ctypes.addressof(outs), ws.data_ptr(), ws.numel(), 0,
                                     ctypes.addressof(opts))
    assert not h.value
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in o.values())  # nothing was launched
    return rc, rcg, err


def test_flag_outside_the_native_set_is_refused():
    """YUMA_RUN_HIST_BF16 where yuma_hist_bf16_native is 0 returns
    YUMA_EUNSUPPORTED before any launch; without B_hist, YUMA_EINVAL."""
    rc, rcg, err = _c_call(Y1, 2, 70, 260, engine.RUN_HIST_BF16, True)
    assert rc == -4 and rcg == -4, (rc, rcg)
    assert b"yuma_hist_bf16_native" in err
    rc, rcg, err = _c_call(Y3, 1, 70, 262, engine.RUN_HIST_BF16, True)  # M % 4 != 0
    assert rc == -4 and rcg == -4, (rc, rcg)
    rc, rcg, err = _c_call(Y3, 2, 70, 260, engine.RUN_HIST_BF16 | engine.RUN_SHARED_INPUTS, True)
    assert rc == -4 and rcg == -4, (rc, rcg)
    rc, rcg, err = _c_call(Y3, 2, 70, 260, engine.RUN_HIST_BF16, False)
    assert rc == -1 and rcg == -1, (rc, rcg)
    assert b"B_hist" in err


def test_run_simulations_bonds_dtype():
    cfg = YumaConfig(simulation=SimulationHyperparameters(bond_penalty=0.99))
    runs = [SimulationRun(builtin_cases[10], "Yuma 3 (Rhef)", cfg)]
    (div, bonds, inc), = run_simulations(runs)
    (div16, bonds16, inc16), = run_simulations(runs, bonds_dtype=BF16)
    assert len(bonds16) == len(bonds) >= 6
    for t, (a, b) in enumerate(zip(bonds16, bonds)):
        assert a.dtype == BF16 and b.dtype == torch.float32
        assert torch.equal(a.view(torch.int16), b.to(BF16).view(torch.int16)), t
    assert div16 == div
    assert all(torch.equal(a, b) for a, b in zip(inc16, inc))
    (_, bonds3, _), = run_simulations(runs, bonds_every=3, bonds_dtype=BF16)
    assert [b.dtype for b in bonds3] == [BF16] * (len(bonds) // 3)
    with pytest.raises(ValueError, match="bonds_dtype"):
        run_simulations(runs, bonds_dtype=torch.float16)
