"""uint16 weight input, host side (CPU only): the C-ABI flag and query
(YUMA_RUN_W_U16, yuma_u16_native), engine.u16_native's native set and its
excluded conditions, and engine.to_u16, the on-chain max-upscale."""

import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from yuma_simulation._internal import engine

Y0, Y1, Y3, Y4 = engine.VARIANT_RUST, engine.VARIANT_YUMA1, engine.VARIANT_YUMA3, engine.VARIANT_YUMA4


def test_header_declares_flag_and_query_and_library_exports_it():
    text = open(os.path.join(ROOT, "include", "yuma_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bYUMA_RUN_W_U16\s*=\s*2\b", code)
    assert re.search(r"\bint\s+yuma_u16_native\s*\(", code)
    assert engine.RUN_W_U16 == 2
    assert hasattr(engine.load_library(), "yuma_u16_native")


@pytest.mark.parametrize("variant,V,M,hist", [(Y3, 256, 4096, True), (Y4, 1024, 64, False)])
def test_native_set(variant, V, M, hist):
    assert engine.u16_native(variant, 1, 10, V, M, hist, ()) is True


@pytest.mark.parametrize("variant,V,M,want,shared", [
    (Y3, 70, 202, (), False),       # M % 4 != 0
    (Y3, 1025, 256, (), False),     # above the register-resident validator count
    (Y1, 70, 260, (), False),       # column-normalised variants
    (Y0, 70, 260, (), False),
    (Y3, 70, 260, ("Wc",), False),  # a materialised matrix
    (Y3, 70, 260, (), True),        # shared inputs
], ids=["M202", "V1025", "yuma1", "yuma0", "Wc", "shared"])
def test_excluded_conditions(variant, V, M, want, shared):
    assert engine.u16_native(variant, 2, 5, V, M, True, want, shared_inputs=shared) is False
    # ... and each is the only thing in the way
    assert engine.u16_native(Y3, 2, 5, 70, 260, True, ()) is True


@pytest.mark.parametrize("name", ["Wn", "Wc", "Wb", "B_inst", "Tv"])
def test_every_materialised_output_is_excluded(name):
    assert not engine.u16_native(Y4, 1, 3, 64, 256, False, (name,))
    assert engine.u16_native(Y4, 1, 3, 64, 256, False, ("D", "R", "P", "T", "Sn", "bond_alpha", "alpha_ab"))


def test_to_u16_row_max_zero_row_and_ties():
    W = torch.tensor([[0.25, 1.0, 0.5, 0.0],
                      [0.0, 0.0, 0.0, 0.0],
                      [3.0, 0.0, 1.5, 0.75]], dtype=torch.float32)
    q = engine.to_u16(W)
    assert q.dtype == torch.uint16 and q.shape == W.shape
    q = q.numpy().astype(np.int64)
    assert q[0].tolist() == [16384, 65535, 32768, 0]  # 16383.75 -> 16384, 32767.5 -> 32768 (even)
    assert q[1].tolist() == [0, 0, 0, 0]
    assert q[2, 0] == 65535 and q[2, 2] == 32768 and q[2, 3] == 16384
    # exact .5 ties go to the even neighbour, both ways
    ties = torch.tensor([[65535.0, 0.5, 1.5, 2.5, 3.5, 32766.5, 32767.5]], dtype=torch.float64)
    assert engine.to_u16(ties).numpy().astype(np.int64).tolist() == [[65535, 0, 2, 2, 4, 32766, 32768]]
    # leading dimensions are batch dimensions: rows are the last axis
    assert engine.to_u16(W.reshape(3, 1, 4)).shape == (3, 1, 4)


def test_to_u16_round_trip_is_identity_on_full_scale_rows():
    rng = np.random.default_rng(7)
    a = rng.integers(0, 65536, size=(5, 33), dtype=np.int64)
    a[:, 3] = 65535
    a[1, :3] = (0, 1, 65534)
    u = torch.from_numpy(a.astype(np.uint16))
    back = engine.to_u16(u.to(torch.float32))
    assert np.array_equal(back.numpy(), u.numpy())


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf")])
def test_to_u16_rejects_bad_input(bad):
    W = torch.tensor([[1.0, 2.0], [bad, 3.0]])
    with pytest.raises(ValueError):
        engine.to_u16(W)
