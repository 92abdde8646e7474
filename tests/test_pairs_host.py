"""Weight pairs, host side (CPU only): the C-ABI symbol yuma_weights_from_pairs
and each of its refusals (made before any HIP call, so they need no GPU),
engine.pairs_from_dense, the integer rounding rule of YUMA_PAIRS_UPSCALE
against engine.to_u16, and engine.weights_from_pairs's own argument checks."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from yuma_simulation._internal import engine

EINVAL = -1


def header_code():
    text = open(os.path.join(ROOT, "include", "yuma_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_and_library_exports_the_entry_point():
    code = header_code()
    assert re.search(r"\bint\s+yuma_weights_from_pairs\s*\(\s*long long rows,\s*int M,\s*long long nnz,", code)
    assert re.search(r"\bYUMA_PAIRS_UPSCALE\s*=\s*1\b", code)
    for name, value in (("DROPPED", 0), ("CONFLICT_ROWS", 1), ("BAD_ROWS", 2), ("WORDS", 4)):
        assert re.search(rf"\bYUMA_PAIRS_ST_{name}\s*=\s*{value}\b", code), name
    assert "yuma_weights_from_pairs" in engine.EXPORTED_SYMBOLS
    assert (engine.PAIRS_UPSCALE, engine.PAIRS_ST_DROPPED, engine.PAIRS_ST_CONFLICT_ROWS, engine.PAIRS_ST_BAD_ROWS,
            engine.PAIRS_ST_WORDS) == (1, 0, 1, 2, 4)
    fn = engine.load_library().yuma_weights_from_pairs
    ll, i32, vp = ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p
    assert list(fn.argtypes) == [ll, i32, ll, vp, vp, vp, i32, vp, vp, vp]
    assert fn.restype is i32


# Dummy non-null pointers on the stated alignments; never dereferenced, since
# every refusal comes before the first launch and rows == 0 launches nothing.
P = 0x1000
# (id, rows, M, nnz, row_ptr, uid, val, flags, W, the argument the text must name)
REFUSALS = [
    ("rows<0", -1, 8, 0, P, P, P, 0, P, "rows"),
    ("M<1", 1, 0, 0, P, P, P, 0, P, "M"),
    ("M<0", 1, -3, 0, P, P, P, 0, P, "M"),
    ("nnz<0", 1, 8, -1, P, P, P, 0, P, "nnz"),
    ("row_ptr", 1, 8, 0, None, P, P, 0, P, "row_ptr"),
    ("W", 1, 8, 0, P, P, P, 0, None, "W"),
    ("uid", 1, 8, 1, P, None, P, 0, P, "uid"),
    ("val", 1, 8, 1, P, P, None, 0, P, "val"),
    ("flag", 1, 8, 0, P, P, P, 2, P, "flags"),
    ("flag-high", 1, 8, 0, P, P, P, 1 | 1 << 20, P, "flags"),
    ("rows*M", (1 << 62) // 8 + 1, 8, 0, P, P, P, 0, P, "rows * M"),
    ("rows*M-wide", 1 << 40, 1 << 30, 0, P, P, P, 0, P, "rows * M"),
]


@pytest.mark.parametrize("rows,M,nnz,rp,uid,val,flags,W,names", [c[1:] for c in REFUSALS],
                         ids=[c[0] for c in REFUSALS])
def test_refusals_come_before_any_launch(rows, M, nnz, rp, uid, val, flags, W, names):
    lib = engine.load_library()
    rc = lib.yuma_weights_from_pairs(rows, M, nnz, rp, uid, val, flags, W, P, None)
    assert rc == EINVAL
    text = lib.yuma_last_error().decode()
    assert names in text, text


def test_null_lists_are_fine_without_pairs_and_zero_rows_is_a_no_op():
    lib = engine.load_library()
    assert lib.yuma_weights_from_pairs(0, 8, 0, None, None, None, 0, None, None, None) == 0
    assert lib.yuma_weights_from_pairs(0, 8, 5, P, P, P, engine.PAIRS_UPSCALE, P, P, None) == 0
    # an earlier refusal still wins over rows == 0
    assert lib.yuma_weights_from_pairs(0, 0, 0, None, None, None, 0, None, None, None) == EINVAL


def test_misaligned_pointers_are_refused():
    lib = engine.load_library()
    for args in ((P + 4, P, P, 0, P, P), (P, P + 1, P, 0, P, P), (P, P, P + 1, 0, P, P), (P, P, P, 0, P + 1, P),
                 (P, P, P, 0, P, P + 2)):
        assert lib.yuma_weights_from_pairs(1, 8, 1, *args, None) == EINVAL
        assert "aligned" in lib.yuma_last_error().decode()


# ---------------------------------------------------------------------------
# pairs_from_dense
# ---------------------------------------------------------------------------
def scatter_dense(row_ptr, uid, val, rows, M):
    """The torch scatter of the lists, row by row (int64 values)."""
    W = torch.zeros(rows, M, dtype=torch.int64)
    u = uid.view(torch.int16).to(torch.int64) & 0xFFFF
    v = val.view(torch.int16).to(torch.int64) & 0xFFFF
    for r in range(rows):
        b, e = int(row_ptr[r]), int(row_ptr[r + 1])
        W[r].scatter_(0, u[b:e], v[b:e])
    return W


def u16(a):
    return torch.from_numpy(np.asarray(a, dtype=np.int64).astype(np.uint16))


def test_pairs_from_dense_round_trip():
    rng = np.random.default_rng(11)
    a = rng.integers(1, 65536, size=(2, 3, 37), dtype=np.int64)
    a[rng.random(a.shape) < 0.7] = 0
    a[0, 1] = 0                                      # an empty row in the middle
    a[1, 2] = rng.integers(1, 65536, size=37)        # a full row at the end
    a[1, 0, 36] = 65535
    row_ptr, uid, val = engine.pairs_from_dense(u16(a))
    assert (row_ptr.dtype, uid.dtype, val.dtype) == (torch.int64, torch.uint16, torch.uint16)
    assert row_ptr.shape == (7,) and uid.shape == val.shape == (int((a != 0).sum()),)
    assert int(row_ptr[0]) == 0 and int(row_ptr[-1]) == uid.numel()
    assert np.array_equal(np.diff(row_ptr.numpy()), (a != 0).reshape(6, 37).sum(1))
    assert int(row_ptr[2]) == int(row_ptr[1]) and int(row_ptr[6]) - int(row_ptr[5]) == 37
    assert (val.view(torch.int16) != 0).all()
    u = uid.numpy().astype(np.int64)
    for r in range(6):  # columns ascending inside every row
        assert np.all(np.diff(u[int(row_ptr[r]):int(row_ptr[r + 1])]) > 0)
    assert np.array_equal(scatter_dense(row_ptr, uid, val, 6, 37).numpy(), a.reshape(6, 37))


def test_pairs_from_dense_all_zero_and_one_dimension():
    row_ptr, uid, val = engine.pairs_from_dense(torch.zeros(4, 5, dtype=torch.uint16))
    assert row_ptr.tolist() == [0] * 5 and uid.numel() == 0 and val.numel() == 0
    assert uid.dtype == torch.uint16 and val.dtype == torch.uint16
    row_ptr, uid, val = engine.pairs_from_dense(u16([0, 7, 0, 65535]))
    assert row_ptr.tolist() == [0, 2]
    assert uid.numpy().tolist() == [1, 3] and val.numpy().tolist() == [7, 65535]


def test_pairs_from_dense_widest_uid_and_refusals():
    W = torch.zeros(1, 65536, dtype=torch.uint16)
    W.view(torch.int16)[0, 65535] = 3
    W.view(torch.int16)[0, 32768] = -1  # 65535
    row_ptr, uid, val = engine.pairs_from_dense(W)
    assert uid.numpy().tolist() == [32768, 65535] and val.numpy().tolist() == [65535, 3]
    with pytest.raises(ValueError, match="65536"):
        engine.pairs_from_dense(torch.zeros(1, 65537, dtype=torch.uint16))
    with pytest.raises(ValueError):
        engine.pairs_from_dense(torch.zeros(2, 4, dtype=torch.int32))


# ---------------------------------------------------------------------------
# the upscale rule
# ---------------------------------------------------------------------------
def upscale_mirror(val, rowmax):
    """YUMA_PAIRS_UPSCALE's rule as the header states it, in Python integers."""
    if rowmax == 0:
        return 0
    n = val * 65535
    q, r = divmod(n, rowmax)
    return q + 1 if 2 * r > rowmax or (2 * r == rowmax and q % 2 == 1) else q


def to_u16_of(vals, rowmax):
    """engine.to_u16 of rows [val, rowmax] (so that the row maximum is rowmax)."""
    rows = torch.tensor([[v, rowmax] for v in vals], dtype=torch.float64)
    return engine.to_u16(rows)[:, 0].numpy().astype(np.int64)


@pytest.mark.parametrize("rowmax", [1, 2, 3, 5, 6, 65534, 65535])
def test_upscale_rule_equals_to_u16_for_every_value(rowmax):
    vals = list(range(rowmax + 1))
    assert to_u16_of(vals, rowmax).tolist() == [upscale_mirror(v, rowmax) for v in vals]


def test_upscale_rule_true_ties_and_random_pairs():
    assert upscale_mirror(1, 2) == 32768 and upscale_mirror(3, 6) == 32768  # 32767.5 -> even
    assert upscale_mirror(1, 6) == 10922 and upscale_mirror(5, 6) == 54612  # 10922.5, 54612.5 -> even
    assert upscale_mirror(0, 0) == 0 and upscale_mirror(7, 7) == 65535
    rng = np.random.default_rng(23)
    mx = rng.integers(1, 65536, size=2000)
    v = (rng.random(2000) * (mx + 1)).astype(np.int64).clip(0, mx)
    rows = torch.from_numpy(np.stack([v, mx], axis=1).astype(np.float64))
    got = engine.to_u16(rows)[:, 0].numpy().astype(np.int64)
    assert got.tolist() == [upscale_mirror(int(a), int(b)) for a, b in zip(v, mx)]


# ---------------------------------------------------------------------------
# weights_from_pairs: what the binding checks itself
# ---------------------------------------------------------------------------
def good():
    return dict(row_ptr=torch.tensor([0, 1, 2], dtype=torch.int64), uid=u16([0, 3]), val=u16([5, 6]), shape=(2, 8))


@pytest.mark.parametrize("change", [
    dict(row_ptr=torch.tensor([0, 1, 2], dtype=torch.int32)),
    dict(row_ptr=torch.tensor([[0, 1, 2]], dtype=torch.int64)),
    dict(row_ptr=torch.tensor([0, 1], dtype=torch.int64)),
    dict(row_ptr=[0, 1, 2]),
    dict(uid=torch.tensor([0, 3], dtype=torch.int16)),
    dict(val=torch.tensor([5, 6], dtype=torch.int32)),
    dict(val=torch.tensor([5.0, 6.0])),
    dict(uid=u16([0, 3, 4])),
    dict(val=u16([5])),
    dict(shape=(3, 8)),
    dict(shape=(2, 0)),
    dict(shape=()),
    dict(shape=(2.0, 8)),
    dict(out=torch.zeros(2, 8, dtype=torch.uint16)),  # not on the device
    dict(stream=0),
], ids=["row_ptr-int32", "row_ptr-2d", "row_ptr-short", "row_ptr-list", "uid-int16", "val-int32", "val-float",
        "uid-long", "val-short", "rows", "M0", "no-shape", "float-shape", "out-cpu", "stream"])
def test_weights_from_pairs_validates_before_the_library(change, monkeypatch):
    def untouched(*a, **k):
        raise AssertionError("the library was reached")

    monkeypatch.setattr(engine, "load_library", untouched)
    monkeypatch.setattr(engine, "device", untouched)
    kw = {**good(), **change}
    with pytest.raises(ValueError):
        engine.weights_from_pairs(kw.pop("row_ptr"), kw.pop("uid"), kw.pop("val"), kw.pop("shape"), **kw)


def test_weights_from_pairs_without_gpu_fails_loudly():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    kw = good()
    with pytest.raises(engine.EngineUnavailable):
        engine.weights_from_pairs(kw["row_ptr"], kw["uid"], kw["val"], kw["shape"])


def test_pairs_status_reads_unsigned_words():
    st = engine.PairsStatus.from_tensor(torch.tensor([3, -1, 7, 0], dtype=torch.int32))
    assert (st.dropped, st.conflict_rows, st.bad_rows) == (3, 0xFFFFFFFF, 7)
