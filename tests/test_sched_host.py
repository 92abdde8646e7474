"""Input schedules, host side (no GPU): the C-ABI of yuma_run_sched and its
companions, the yuma_sched_native truth table, the workspace size, the
bit-exact slice dedup and the schedule validation of engine.run (which raises
before anything touches a device)."""

from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest
import torch

from yuma_simulation._internal import engine
from yuma_simulation._internal.yumas import YumaConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("yuma_workspace_bytes_sched", "yuma_run_sched", "yuma_graph_create_sched", "yuma_sched_native")
RUST, Y1, Y2, Y3, Y4 = range(5)


def header_code():
    text = open(os.path.join(ROOT, "include", "yuma_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def proto(name):
    return re.search(r"\b(\w+)\s+" + name + r"\s*\((.*?)\)\s*;", header_code(), flags=re.S)


def test_header_declares_the_entry_points():
    code = header_code()
    assert proto("yuma_workspace_bytes_sched").group(1) == "size_t"
    for name in NEW_FUNCTIONS[1:]:
        assert proto(name).group(1) == "int", name
    for name in ("yuma_run_sched", "yuma_graph_create_sched"):
        args = proto(name).group(2)
        assert "const int32_t* sched_dev" in args and "int K" in args, name
        assert "const yuma_run_options_t* opts" in args, name
    # the options record is untouched: its reserved words stay reserved
    assert re.search(r"int32_t\s+reserved\[5\]\s*;", code)
    assert re.search(r"YUMA_NUM_PHASES\s*=\s*7\b", code)


def n_params(name):
    return len([a for a in proto(name).group(2).split(",") if a.strip()])


def test_library_exports_and_argtypes_match_the_header():
    lib = engine.load_library()
    for name in NEW_FUNCTIONS:
        assert name in engine.EXPORTED_SYMBOLS, name
        fn = getattr(lib, name)
        assert len(fn.argtypes) == n_params(name), name
    assert lib.yuma_workspace_bytes_sched.restype is ctypes.c_size_t
    # yuma_run_sched is yuma_run_opts with K after E and the schedule after S
    a, b = list(lib.yuma_run_opts.argtypes), list(lib.yuma_run_sched.argtypes)
    assert b == a[:4] + [ctypes.c_int] + a[4:8] + [ctypes.c_void_p] + a[8:]
    a, b = list(lib.yuma_graph_create_opts.argtypes), list(lib.yuma_graph_create_sched.argtypes)
    assert b == a[:5] + [ctypes.c_int] + a[5:9] + [ctypes.c_void_p] + a[9:]
    assert list(lib.yuma_sched_native.argtypes) == [ctypes.c_int] * 6 + [ctypes.c_void_p, ctypes.c_int]


@pytest.mark.parametrize("V,M", [(70, 260), (engine.MAX_VALIDATORS, 64)])
def test_sched_native_truth_table(V, M):
    N, E, K = 2, 11, 3
    for variant in (Y3, Y4):
        assert engine.sched_native(variant, N, E, K, V, M)
        assert engine.sched_native(variant, N, E, K, V, M, want_hist=True, want=("D", "R", "Sn", "bond_alpha", "alpha_ab"))
        assert engine.sched_native(variant, N, E, 40, V, M)  # K > E
        assert not engine.sched_native(variant, N, E, K, V, M + 2)
        assert not engine.sched_native(variant, N, E, K, V, M, shared_inputs=True)
        for name in ("Wn", "Wc", "Wb", "B_inst", "Tv", "P", "T"):
            assert not engine.sched_native(variant, N, E, K, V, M, want=(name,)), name
        # with uint16 weights it follows yuma_u16_native
        for want in ((), ("Wn",)):
            assert (engine.sched_native(variant, N, E, K, V, M, want=want, w_u16=True)
                    == engine.u16_native(variant, N, E, V, M, want=want))
        assert engine.sched_native(variant, N, E, K, V, M, w_u16=True) == (V <= engine.REG_VALIDATORS)
        # ... and with a bfloat16 history yuma_hist_bf16_native (a history must be wanted)
        assert engine.sched_native(variant, N, E, K, V, M, want_hist=True, hist_bf16=True)
        assert not engine.sched_native(variant, N, E, K, V, M, want_hist=False, hist_bf16=True)
    for variant in (RUST, Y1, Y2):
        assert not engine.sched_native(variant, N, E, K, V, M)
    assert not engine.sched_native(Y3, N, E, 0, V, M)
    assert not engine.sched_native(Y3, N, E, K, engine.MAX_VALIDATORS + 1, M)


def test_native_queries_of_the_other_features_keep_their_answers():
    assert engine.u16_native(Y3, 2, 11, 70, 260) and not engine.u16_native(Y3, 2, 11, 1100, 64)
    assert engine.hist_bf16_native(Y4, 2, 11, 1100, 64) and not engine.hist_bf16_native(Y1, 2, 11, 70, 260)


def test_workspace_bytes_sched():
    lib = engine.load_library()
    for variant in (Y3, Y4):
        for N, E, V, M in ((2, 11, 70, 260), (1, 11, 12, 1024), (1, 11, 1100, 64), (1, 1000, 256, 4096)):
            dense = engine.workspace_bytes(variant, N, E, V, M, False)
            sizes = [engine.workspace_bytes_sched(variant, N, E, K, V, M, False) for K in (1, 2, 3, 10, E, 4 * E)]
            assert sizes[0] >= dense
            assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]
            # the staging set leaves out the bond state and the dividend partials: K = E costs less than twice
            assert sizes[4] < 2 * dense
    assert lib.yuma_workspace_bytes_sched(Y3, 2, 11, 0, 70, 260, 0) == 0


def bits(t):
    return engine._int_view(t.contiguous())


def make_slices(E, N=2, V=5, M=8, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((E, N, V, M), generator=g), torch.rand((E, N, V), generator=g) + 0.5


def check_reproduces(W, S, Wk, Sk, sched):
    assert sched.dtype == torch.int32 and tuple(sched.shape) == (W.shape[0],)
    assert Wk.dtype == W.dtype and Sk.dtype == S.dtype
    idx = sched.long()
    assert torch.equal(bits(Wk)[idx], bits(W))
    assert torch.equal(bits(Sk)[idx], bits(S))
    # order of first occurrence: the first use of slice k comes after that of k - 1
    first = [int((sched == k).nonzero()[0]) for k in range(Wk.shape[0])]
    assert first == sorted(first) and len(set(first)) == len(first)


def test_dedup_identity_and_all_equal():
    W, S = make_slices(6)
    Wk, Sk, sched = engine.dedup_slices(W, S)
    assert sched.tolist() == list(range(6)) and torch.equal(bits(Wk), bits(W)) and torch.equal(bits(Sk), bits(S))
    W1, S1 = W[:1].expand(7, -1, -1, -1), S[:1].expand(7, -1, -1)
    Wk, Sk, sched = engine.dedup_slices(W1, S1)
    assert Wk.shape[0] == 1 and Sk.shape[0] == 1 and sched.tolist() == [0] * 7
    check_reproduces(W1.contiguous(), S1.contiguous(), Wk, Sk, sched)


def test_dedup_abab_and_out_of_order():
    W, S = make_slices(3)
    pick = [0, 1, 0, 1]
    Wk, Sk, sched = engine.dedup_slices(W[pick], S[pick])
    assert Wk.shape[0] == 2 and sched.tolist() == [0, 1, 0, 1]
    check_reproduces(W[pick], S[pick], Wk, Sk, sched)
    # first occurrence decides the order, whatever the slices' sort order
    pick = [2, 2, 0, 0, 0, 1, 1, 2, 0, 1, 1]
    Wk, Sk, sched = engine.dedup_slices(W[pick], S[pick])
    assert sched.tolist() == [0, 0, 1, 1, 1, 2, 2, 0, 1, 2, 2]
    assert torch.equal(Wk, W[[2, 0, 1]]) and torch.equal(Sk, S[[2, 0, 1]])


def test_dedup_slices_differing_only_in_stake_or_in_one_weight():
    W, S = make_slices(1)
    W4, S4 = W.repeat(4, 1, 1, 1), S.repeat(4, 1, 1)
    S4[2, 1, 3] += 0.25
    W4[3, 0, 4, 7] += 0.125
    Wk, Sk, sched = engine.dedup_slices(W4, S4)
    assert sched.tolist() == [0, 0, 1, 2]
    check_reproduces(W4, S4, Wk, Sk, sched)


def test_dedup_keeps_signed_zeros_and_nan_payloads_apart():
    W, S = make_slices(1)
    W3, S3 = W.repeat(3, 1, 1, 1), S.repeat(3, 1, 1)
    W3[:, 0, 0, 0] = torch.tensor([0.0, -0.0, 0.0])
    Wk, Sk, sched = engine.dedup_slices(W3, S3)
    assert sched.tolist() == [0, 1, 0]
    check_reproduces(W3, S3, Wk, Sk, sched)
    nan_a = torch.tensor([0x7FC00000, 0x7FC00001, 0x7FC00000], dtype=torch.int32).view(torch.float32)
    W3[:, 0, 0, 0] = nan_a
    Wk, Sk, sched = engine.dedup_slices(W3, S3)
    assert sched.tolist() == [0, 1, 0]
    check_reproduces(W3, S3, Wk, Sk, sched)


def test_dedup_uint16_weights():
    g = torch.Generator().manual_seed(5)
    W = torch.randint(0, 65536, (3, 2, 5, 8), generator=g).to(torch.uint16)
    S = torch.rand((3, 2, 5), generator=g)
    pick = torch.tensor([1, 1, 0, 2, 0])
    Wp = W.view(torch.int16)[pick].view(torch.uint16)
    Wk, Sk, sched = engine.dedup_slices(Wp, S[pick])
    assert Wk.dtype == torch.uint16 and sched.tolist() == [0, 0, 1, 2, 1]
    check_reproduces(Wp, S[pick], Wk, Sk, sched)


def test_dedup_rejects_mismatched_shapes():
    W, S = make_slices(3)
    with pytest.raises(ValueError):
        engine.dedup_slices(W, S[:2])
    with pytest.raises(ValueError):
        engine.dedup_slices(W[0], S[0])


# ---------------------------------------------------------------------------
# engine.run validates the schedule on the host, before it asks for a device
# ---------------------------------------------------------------------------
def run_args(K=3, N=2, V=5, M=8):
    W, S = make_slices(K, N, V, M)
    return Y3, [engine.make_params(Y3, YumaConfig())] * N, W, S


@pytest.fixture()
def no_device(monkeypatch):
    """Any request for the device fails the test: validation comes first."""
    def boom():
        raise AssertionError("engine.run asked for a device before validating the schedule")
    monkeypatch.setattr(engine, "device", boom)


@pytest.mark.parametrize("sched", [
    pytest.param([], id="empty"),
    pytest.param([[0, 1], [1, 2]], id="two-dimensional"),
    pytest.param([0, 1, -1, 2], id="negative"),
    pytest.param([0, 1, 3, 2], id="entry-K"),
    pytest.param([0.0, 1.0, 2.0], id="float-list"),
    pytest.param(torch.tensor([0.0, 1.0]), id="float-tensor"),
    pytest.param(torch.tensor([True, False]), id="bool-tensor"),
    pytest.param(np.array([0, 1, 2 ** 40]), id="beyond-int32"),
])
def test_run_rejects_a_bad_schedule_before_touching_the_device(no_device, sched):
    variant, params, W, S = run_args()
    with pytest.raises(ValueError, match="sched"):
        engine.run(variant, params, W, S, sched=sched)


def test_run_rejects_a_schedule_of_the_wrong_length_for_the_callers_outputs(no_device):
    variant, params, W, S = run_args()
    out = {"Dn": torch.empty((11, 2, 5))}
    with pytest.raises(ValueError, match="epochs"):
        engine.run(variant, params, W, S, sched=[0, 1, 2, 0, 1], out=out)


def test_run_rejects_stakes_that_are_not_per_stored_slice(no_device):
    variant, params, W, S = run_args()
    sched = [0, 1, 2, 2, 1]
    with pytest.raises(ValueError, match=r"S shape"):
        engine.run(variant, params, W, S[sched], sched=sched)  # S expanded, W not
    with pytest.raises(ValueError, match=r"S shape"):
        engine.run(variant, params, W, S[:, :, :4], sched=sched)


def test_a_valid_schedule_passes_validation():
    h = engine._sched_host(torch.tensor([2, 0, 1, 1], dtype=torch.int32), 3)
    assert h.dtype == torch.int64 and h.tolist() == [2, 0, 1, 1]
    assert engine._sched_host((0, 0, 0), 1).tolist() == [0, 0, 0]
    assert engine._sched_host(np.array([1, 0], dtype=np.uint8), 2).tolist() == [1, 0]
