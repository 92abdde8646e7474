"""bfloat16 bond history, host side (no GPU): the C-ABI flag and query
(YUMA_RUN_HIST_BF16, yuma_hist_bf16_native), the query's native set and its
excluded conditions, the flag's acceptance by the options check, and the
argument checks of engine.run that come before any device work."""

from __future__ import annotations

import ctypes
import os
import re

import pytest
import torch

from yuma_simulation._internal import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Y0, Y1, Y2, Y3, Y4 = (engine.VARIANT_RUST, engine.VARIANT_YUMA1, engine.VARIANT_YUMA2, engine.VARIANT_YUMA3,
                      engine.VARIANT_YUMA4)
# the argument tuple of test_hist_stride_host.test_bad_options_return_einval_before_any_launch
RUN_ARGS = (3, None, 1, 11, 8, 64, None, None, None, None, None, None, 0, 0)


def test_header_declares_the_flag_and_the_query():
    text = open(os.path.join(ROOT, "include", "yuma_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bYUMA_RUN_HIST_BF16\s*=\s*4\b", code)
    assert re.search(r"\bint\s+yuma_hist_bf16_native\s*\(", code)
    # the entry points that stay fp32 are named where the flag is described
    doc = text[:text.index("enum yuma_run_flags")]
    doc = doc[doc.rindex("YUMA_RUN_HIST_BF16 "):]
    for name in ("yuma_epoch", "yuma_run", "yuma_graph_create", "yuma_shard_stage"):
        assert name in doc, name


def test_library_exports_the_query():
    lib = engine.load_library()
    assert engine.RUN_HIST_BF16 == 4
    assert hasattr(lib, "yuma_hist_bf16_native")
    assert len(lib.yuma_hist_bf16_native.argtypes) == 7
    # (engine.EXPORTED_SYMBOLS mirrors the header scan of tests/test_host.py, whose
    # pattern takes names of lower-case letters only: like yuma_u16_native, the
    # query is typed in load_library and stays outside that tuple)
    assert lib.yuma_hist_bf16_native.argtypes == lib.yuma_u16_native.argtypes


@pytest.mark.parametrize("variant,V,M", [(Y3, 70, 260), (Y4, 1100, 96), (Y3, 256, 4096)])
def test_native_set(variant, V, M):
    assert engine.hist_bf16_native(variant, 2, 11, V, M) is True


@pytest.mark.parametrize("variant,M,kw", [
    (Y3, 262, {}),                        # M % 4 != 0: the scalar scan
    (Y0, 260, {}), (Y1, 260, {}), (Y2, 260, {}),  # the column-normalised variants
    (Y3, 260, {"shared_inputs": True}),   # k_bonds_grp
    (Y3, 260, {"want_hist": False}),      # no B_hist requested
], ids=["M262", "yuma0", "yuma1", "yuma2", "shared", "nohist"])
def test_excluded_conditions(variant, M, kw):
    assert engine.hist_bf16_native(variant, 2, 11, 70, M, **kw) is False
    # ... and each is the only thing in the way
    assert engine.hist_bf16_native(Y3, 2, 11, 70, 260) is True


def test_query_reads_only_b_hist_of_the_outputs_and_takes_null():
    lib = engine.load_library()
    assert lib.yuma_hist_bf16_native(Y3, 2, 11, 70, 260, None, 0) == 0
    outs = engine.YumaOutputsC(**{k: 1 for k in engine.OUTPUT_FIELDS})
    assert lib.yuma_hist_bf16_native(Y4, 2, 11, 70, 260, ctypes.addressof(outs), 0) == 1
    assert lib.yuma_hist_bf16_native(Y4, 2, 11, 70, 260, ctypes.addressof(outs), engine.RUN_W_U16) == 1
    assert lib.yuma_hist_bf16_native(Y4, 2, 11, 70, 260, ctypes.addressof(outs), engine.RUN_SHARED_INPUTS) == 0
    assert lib.yuma_hist_bf16_native(Y4, 2, 11, engine.MAX_VALIDATORS, 64, ctypes.addressof(outs), 0) == 1
    assert lib.yuma_hist_bf16_native(Y4, 2, 11, engine.MAX_VALIDATORS + 1, 64, ctypes.addressof(outs), 0) == 0


def test_flag_is_a_known_run_flag():
    """flags = 4 passes the options check: the call goes on to the null
    pointers and fails on those. (Before the flag existed the text was
    "unknown run flags 0x4".)"""
    lib = engine.load_library()
    for flags in (engine.RUN_HIST_BF16, engine.RUN_HIST_BF16 | engine.RUN_W_U16):
        opts = engine.YumaRunOptionsC(flags=flags, hist_stride=3, hist_first=2)
        rc = lib.yuma_run_opts(*RUN_ARGS, ctypes.addressof(opts), None, None)
        assert rc < 0
        assert "unknown run flags" not in lib.yuma_last_error().decode()
        h = ctypes.c_void_p()
        rc = lib.yuma_graph_create_opts(ctypes.byref(h), *RUN_ARGS, ctypes.addressof(opts))
        assert rc < 0 and not h.value
        assert "unknown run flags" not in lib.yuma_last_error().decode()
        rc = lib.yuma_run_ex(*RUN_ARGS, flags, None, None)
        assert rc < 0
        assert "unknown run flags" not in lib.yuma_last_error().decode()


def test_unknown_flag_is_still_refused():
    lib = engine.load_library()
    opts = engine.YumaRunOptionsC(flags=1 << 10)
    assert lib.yuma_run_opts(*RUN_ARGS, ctypes.addressof(opts), None, None) == -1
    assert "unknown run flags" in lib.yuma_last_error().decode()
    opts = engine.YumaRunOptionsC(flags=engine.RUN_HIST_BF16 | 8)
    assert lib.yuma_run_opts(*RUN_ARGS, ctypes.addressof(opts), None, None) == -1
    assert "unknown run flags" in lib.yuma_last_error().decode()
    assert lib.yuma_run_ex(*RUN_ARGS, 1 << 10, None, None) == -1


def test_options_record_keeps_its_layout():
    assert ctypes.sizeof(engine.YumaRunOptionsC) == 32
    opts = engine.YumaRunOptionsC(flags=engine.RUN_HIST_BF16, reserved=(0, 0, 0, 1, 0))
    assert engine.load_library().yuma_run_opts(*RUN_ARGS, ctypes.addressof(opts), None, None) == -1
    assert "reserved" in engine.load_library().yuma_last_error().decode()


def test_run_checks_hist_dtype_before_any_device_work():
    """ValueError with or without a GPU: the dtype checks come first."""
    W = torch.zeros((1, 1, 4, 8))
    S = torch.ones((1, 1, 4))
    for bad in (torch.float16, torch.float64, torch.int16, "bfloat16"):
        with pytest.raises(ValueError, match="hist_dtype"):
            engine.run(Y3, [], W, S, want_hist=True, hist_dtype=bad)
    with pytest.raises(ValueError, match="single_call"):
        engine.run(Y3, [], W, S, want_hist=True, hist_dtype=torch.bfloat16, single_call=True)
