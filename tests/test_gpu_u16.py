"""uint16 weight input on the GPU (gpu marker): engine.run / engine.RunGraph on
a torch.uint16 W take the native path (YUMA_RUN_W_U16: 8-byte loads converted
in registers) and return, array for array, the bits of the same call on
W.to(torch.float32) -- (float)w is exact, and the arithmetic behind the load is
the fp32 kernels' own. Outside the native set the binding widens W and says so.

Weights: seeded integers over 0..65535, about 10 % zeros, every row with one
65535 and one more value >= 32768, so a sign-extending or 15-bit load cannot
pass. Shapes: the smallest that reach each load path and edge (see CASES)."""

import ctypes

import numpy as np
import pytest
import torch

from conftest import assert_close
from oracle import yuma_oracle as orc

pytestmark = pytest.mark.gpu

from yuma_simulation._internal import engine, synth  # noqa: E402
from yuma_simulation._internal.yumas import (  # noqa: E402
    SimulationHyperparameters,
    YumaConfig,
    YumaParams,
)

Y1, Y3, Y4 = engine.VARIANT_YUMA1, engine.VARIANT_YUMA3, engine.VARIANT_YUMA4
WANT = ("D", "R", "Sn", "bond_alpha", "alpha_ab")
ZERO_COL = 100  # the zeroed miner column of the reset case (never a row's 65535 / >= 32768 column)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "gpu tests need a ROCm GPU"
    engine.load_library()
    yield


def weights_u16(seed, E, N, V, M, zero=None):
    """[E, N, V, M] uint16 (numpy): uniform over 0..65535, ~10 % zeros; row v
    holds 65535 at column v % 8 and a value >= 32768 at column 8 + v % 8.
    zero = (epoch, column): that miner column is all zero in that epoch."""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 65536, size=(E, N, V, M), dtype=np.int64)
    w[rng.random((E, N, V, M)) < 0.1] = 0
    v = np.arange(V)
    w[:, :, v, v % 8] = 65535
    w[:, :, v, 8 + v % 8] = 32768 + (w[:, :, v, 8 + v % 8] >> 1)
    assert ((w == 65535).any(-1) & ((w >= 32768) & (w < 65535)).any(-1)).all()
    if zero is not None:
        w[zero[0], :, :, zero[1]] = 0
    return w.astype(np.uint16)


def config(liquid=False):
    return YumaConfig(simulation=SimulationHyperparameters(bond_penalty=0.99),
                      yuma_params=YumaParams(liquid_alpha=liquid))


def inputs(seed, E, N, V, M, zero=None):
    W = torch.from_numpy(weights_u16(seed, E, N, V, M, zero))
    S = torch.from_numpy(synth.stakes(seed, E, N, V, period=2))
    return W, S


def assert_same_bits(a, b, hist, want=WANT):
    torch.cuda.synchronize()
    names = ["Dn", "C", "I", "B_final"] + (["B_hist"] if hist else [])
    for k in names:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    for k in want:
        # (NaN-free: bond_alpha / alpha_ab are requested for liquid runs only)
        assert torch.equal(a.extra[k], b.extra[k]), k


def run_pair(variant, params, W, S, hist, want=WANT, **kw):
    """The uint16 call and the same call on the widened tensor."""
    a = engine.run(variant, params, W, S, want_hist=hist, want=want, **kw)
    b = engine.run(variant, params, W.to(torch.float32), S, want_hist=hist, want=want, **kw)
    assert b.extra["w_path"] == "f32"
    return a, b


# (id, variant, E, N, V, M, hist, chunk_epochs): what each shape reaches
CASES = [
    ("min-y3", Y3, 4, 1, 3, 64, True, 0),          # minimal
    ("min-y4", Y4, 4, 1, 3, 64, True, 0),
    # M % 8 != 0: rows 8- but not 16-byte aligned; ragged row group; tile
    # edge; slice and chunk offsets in 2-byte units across N and chunks
    ("ragged", Y3, 5, 2, 70, 260, True, 2),
    ("wide-hist", Y3, 3, 1, 256, 1024, True, 0),   # the 512-thread wide-history scan
    ("one-row", Y3, 3, 1, 256, 1024, False, 0),    # the one-row history-less scan
    # wide k_rowsum (>= 64 chunks), two rows per lane (>= 4096 blocks), wide rank
    ("wide-rows", Y4, 2, 1, 256, 32768, False, 0),
    ("v1024", Y3, 2, 1, 1024, 128, True, 0),       # the widest register-resident consensus / rank
]


@pytest.mark.parametrize("variant,E,N,V,M,hist,chunk", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_native_run_has_the_fp32_bits(variant, E, N, V, M, hist, chunk):
    W, S = inputs(0x16 + V + M, E, N, V, M)
    params = [engine.make_params(variant, config())] * N
    want = ("D", "R", "Sn")  # scalar alpha: bond_alpha / alpha_ab are not written
    a, b = run_pair(variant, params, W, S, hist, want=want, chunk_epochs=chunk)
    assert a.extra["w_path"] == "u16"
    assert a.extra["_inputs"][0].dtype == torch.uint16  # W stayed 16-bit on the device
    assert_same_bits(a, b, hist, want)
    assert float(a.Dn.sum()) > 0 and float(a.B_final.abs().sum()) > 0


@pytest.fixture(scope="module")
def ragged():
    """The 70 x 260 case (Yuma 3, history, chunks of 2) and its oracle runs."""
    E, N, V, M = 5, 2, 70, 260
    W, S = inputs(0x70260, E, N, V, M)
    cfg = config()
    params = [engine.make_params(Y3, cfg)] * N
    ref = [orc.run("Yuma 3 (Rhef)", W[:, n].numpy().astype(np.float32), S[:, n].numpy(), cfg) for n in range(N)]
    return W, S, params, ref


def check_oracle(res, ref, n, tag):
    np.testing.assert_array_equal(res.C[:, n].cpu().numpy(), ref["C"], err_msg=tag)
    assert_close(res.Dn[:, n].cpu().numpy(), ref["Dn"], what=f"{tag} Dn")
    assert_close(res.I[:, n].cpu().numpy(), ref["I"], what=f"{tag} I")
    assert_close(res.B_hist[:, n].cpu().numpy(), ref["B"], what=f"{tag} B")


def test_ragged_matches_oracle(ragged):
    W, S, params, ref = ragged
    a = engine.run(Y3, params, W, S, want_hist=True, chunk_epochs=2)
    torch.cuda.synchronize()
    assert a.extra["w_path"] == "u16"
    for n in range(2):
        check_oracle(a, ref[n], n, f"70x260 scenario {n}")


def test_view_at_8_byte_offset_stays_native(ragged):
    """W a contiguous view 4 elements into a larger device buffer: the base is
    8- but not 16-byte aligned, which the uint16 loads must take as it is."""
    W, S, params, _ = ragged
    dev = engine.device()
    buf = torch.empty(W.numel() + 8, dtype=torch.uint16, device=dev)
    view = buf[4:4 + W.numel()].view(W.shape)
    view.copy_(W.to(dev))
    assert view.data_ptr() % 16 == 8 and view.is_contiguous()
    a = engine.run(Y3, params, view, S, want_hist=True, want=("D", "R", "Sn"), chunk_epochs=2)
    b = engine.run(Y3, params, W.to(torch.float32), S, want_hist=True, want=("D", "R", "Sn"), chunk_epochs=2)
    assert a.extra["w_path"] == "u16"
    assert a.extra["_inputs"][0].data_ptr() == view.data_ptr()
    assert_same_bits(a, b, True, ("D", "R", "Sn"))


def test_liquid_yuma4_with_conditional_reset():
    """Yuma 4 liquid alpha, reset_mode IF_ZERO_CONSENSUS at epoch 3 on a column
    zeroed at epoch 2 (C = 0 there, so the reset fires): fp32 bits, and the
    oracle under the parity contract."""
    E, N, V, M = 6, 1, 64, 256
    W, S = inputs(0x64256, E, N, V, M, zero=(2, ZERO_COL))
    cfg = config(liquid=True)
    params = [engine.make_params(Y4, cfg, reset_mode=engine.RESET_IF_ZERO_CONSENSUS, reset_epoch=3,
                                 reset_index=ZERO_COL, n_miners=M, n_epochs=E)]
    a, b = run_pair(Y4, params, W, S, True)
    assert a.extra["w_path"] == "u16"
    assert_same_bits(a, b, True)
    assert (a.C[2, :, ZERO_COL] == 0).all()
    assert (a.B_hist[3, 0, :, ZERO_COL] != a.B_hist[2, 0, :, ZERO_COL]).any()
    version = "Yuma 4 (Rhef+relative bonds) - liquid alpha on"
    Wf, Sf = W[:, 0].numpy().astype(np.float32), S[:, 0].numpy()
    ref = orc.run(version, Wf, Sf, cfg, reset_epoch=3, reset_index=ZERO_COL)
    check_oracle(a, ref, 0, "64x256 liquid reset")
    ref0 = orc.run(version, Wf, Sf, cfg)  # the reset fired: without it the column's bonds differ
    assert not np.allclose(ref0["B"][3][:, ZERO_COL], ref["B"][3][:, ZERO_COL])


def test_graph_replay_and_refill(ragged):
    W, S, params, _ = ragged
    dev = engine.device()
    Wd = W.to(dev)
    direct = engine.run(Y3, params, Wd, S, want_hist=True, chunk_epochs=2)
    g = engine.RunGraph(Y3, params, Wd, S, want_hist=True, chunk_epochs=2)
    try:
        assert g.result.extra["w_path"] == "u16"
        assert g.result.extra["_inputs"][0].data_ptr() == Wd.data_ptr()
        r = g.launch()
        assert_same_bits(r, direct, True, ())
        W2 = torch.from_numpy(weights_u16(0x2222, *W.shape)).to(dev)
        Wd.copy_(W2)  # refill the captured input in place
        r = g.launch()
        fresh = engine.run(Y3, params, W2.clone(), S, want_hist=True, chunk_epochs=2)
        assert_same_bits(r, fresh, True, ())
        assert not torch.equal(fresh.B_final, direct.B_final)
    finally:
        g.close()


@pytest.mark.parametrize("what", ["M202", "yuma1", "shared", "Wc"])
def test_fallbacks_widen_and_say_so(what):
    variant, E, N, V, M, want, kw = Y3, 5, 2, 70, 260, ("D", "R", "Sn"), {}
    if what == "M202":
        M = 202
    elif what == "yuma1":
        variant = Y1
    elif what == "shared":
        kw = {"shared_inputs": True}
    else:
        want = ("Wc",)
    W, S = inputs(0xFA11, E, 1 if what == "shared" else N, V, M)
    params = [engine.make_params(variant, config())] * N
    a, b = run_pair(variant, params, W, S, True, want=want, **kw)
    assert a.extra["w_path"] == "f32"
    assert a.extra["_inputs"][0].dtype == torch.float32
    assert_same_bits(a, b, True, want)


@pytest.mark.skipif(not hasattr(engine, "RUN_W_U16"), reason="an engine without the uint16 flag")
def test_flag_outside_the_native_set_is_refused():
    """yuma_run_ex with YUMA_RUN_W_U16 where yuma_u16_native is 0 returns
    YUMA_EUNSUPPORTED before any launch. Every pointer is valid and sized for
    fp32 (M = 202), so the call could only read in bounds."""
    E, N, V, M = 2, 1, 8, 202
    assert not engine.u16_native(Y3, N, E, V, M, False, ())
    dev = engine.device()
    lib = engine.load_library()
    W = torch.ones((E, N, V, M), dtype=torch.float32, device=dev)
    S = torch.ones((E, N, V), dtype=torch.float32, device=dev)
    prm = engine.params_tensor([engine.make_params(Y3, config())], dev)
    o = {k: torch.full(s, -7.0, dtype=torch.float32, device=dev)
         for k, s in (("Dn", (E, N, V)), ("C", (E, N, M)), ("I", (E, N, M)), ("B_final", (N, V, M)))}
    outs = engine.YumaOutputsC(**{k: (o[k].data_ptr() if k in o else None) for k in engine.OUTPUT_FIELDS})
    ws = torch.empty(engine.workspace_bytes(Y3, N, E, V, M, False), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rc = lib.yuma_run_ex(Y3, prm.data_ptr(), N, E, V, M, W.data_ptr(), S.data_ptr(), None, None,
                         ctypes.addressof(outs), ws.data_ptr(), ws.numel(), 0, engine.RUN_W_U16, stream, None)
    assert rc == -4, rc  # YUMA_EUNSUPPORTED
    assert b"yuma_u16_native" in lib.yuma_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == -7.0).all()) for t in o.values())  # nothing was launched
