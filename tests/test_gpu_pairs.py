"""Weight pairs on the GPU (gpu marker): engine.weights_from_pairs builds the
dense uint16 W of CSR (uid, weight) lists on the device
(yuma_weights_from_pairs: status zero, fill, scatter, read-back).

Reference: a CPU scatter of the lists, row by row, with the documented rules
(uid >= M dropped, ranges clamped); with upscale, engine.to_u16 of that dense
tensor. Every comparison is bit equality of the whole W.

Shapes: M = 8 (one 16-byte store per row), 12 (M % 8 != 0: the 2-byte fill),
264 (several stores per row; rows of 200, 64 and 65 pairs: one and two 64-lane
passes and the boundary between them), 4096 (a single row). Each also into an
`out` view one element into a buffer: unaligned, so the 2-byte fill at
M % 8 == 0. rows = 1, 3 and 1030: the scatter and read-back grids hold at most
GRID_WAVES = 1024 waves (kPairsWaves in the engine source: 256 blocks of 4), a
row per wave, so at 1030 rows the waves 0..5 take a second row through the
grid-stride loop."""

import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from yuma_simulation._internal import engine, synth  # noqa: E402
from yuma_simulation._internal.yumas import SimulationHyperparameters, YumaConfig, YumaParams  # noqa: E402

Y3, Y4 = engine.VARIANT_YUMA3, engine.VARIANT_YUMA4
GRID_WAVES = 1024
MANY = 1030
assert MANY > GRID_WAVES


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "gpu tests need a ROCm GPU"
    engine.load_library()
    yield


# ---------------------------------------------------------------------------
# lists and their reference
# ---------------------------------------------------------------------------
def t_u16(a):
    return torch.from_numpy(np.asarray(a, dtype=np.int64).astype(np.uint16))


def lists_of(rows_pairs):
    """(row_ptr, uid, val) as int64 numpy arrays from a list of rows, each a list of (uid, val)."""
    row_ptr = np.zeros(len(rows_pairs) + 1, dtype=np.int64)
    row_ptr[1:] = np.cumsum([len(r) for r in rows_pairs])
    flat = [p for r in rows_pairs for p in r]
    uid = np.array([p[0] for p in flat], dtype=np.int64)
    val = np.array([p[1] for p in flat], dtype=np.int64)
    return row_ptr, uid, val


def clamp(row_ptr, nnz):
    """The engine's rule: start into [0, nnz], end into [start, nnz]; the rows that moved."""
    b = np.clip(row_ptr[:-1], 0, nnz)
    e = np.clip(np.maximum(row_ptr[1:], b), None, nnz)
    return b, e, (b != row_ptr[:-1]) | (e != row_ptr[1:])


def reference(row_ptr, uid, val, rows, M, upscale=False):
    """CPU scatter, row by row (a later duplicate overwrites an earlier one); uint16 torch tensor [rows, M]."""
    b, e, _ = clamp(row_ptr, len(uid))
    W = torch.zeros(rows, M, dtype=torch.int64)
    u, v = torch.from_numpy(uid), torch.from_numpy(val)
    for r in range(rows):
        ur, vr = u[b[r]:e[r]], v[b[r]:e[r]]
        keep = ur < M
        W[r].scatter_(0, ur[keep], vr[keep])
    if upscale:
        return engine.to_u16(W.to(torch.float64))
    return t_u16(W.numpy())


def pair_counts(rows, M, rng):
    c = rng.integers(0, min(M, 24) + 1, size=rows)
    if rows == 1:
        c[:] = M if M == 4096 else min(M, 5)
    elif rows == 3:
        c[:] = (min(M, 200), min(M, 64), min(M, 65)) if M >= 64 else (M, 0, 3)
    else:
        c[[0, rows // 2, rows - 1]] = 0                              # empty rows: start, middle, end
        c[1:4] = (min(M, 200), min(M, 64), min(M, 65))               # one, exactly one and two 64-lane passes
        c[4] = c[rows - 3] = M                                       # every column; the second beyond GRID_WAVES
    return c


@functools.lru_cache(maxsize=None)
def case(rows, M):
    """Seeded lists of a shape and both references; treated as read-only by every test."""
    rng = np.random.default_rng(1000 * rows + M)
    out = []
    for r, k in enumerate(pair_counts(rows, M, rng)):
        uids = rng.permutation(M)[:k]                                # shuffled, no duplicates
        if r % 3 == 1:
            uids = np.sort(uids)[::-1]                               # descending
        vals = rng.integers(1, 65535, size=k)
        if k >= 2:
            vals[1] = 0                                              # a val == 0 pair
            if r % 2 == 0:
                vals[0] = 65535                                      # (odd rows keep a smaller maximum for upscale)
        out.append(list(zip(uids.tolist(), vals.tolist())))
    row_ptr, uid, val = lists_of(out)
    return (row_ptr, uid, val, reference(row_ptr, uid, val, rows, M), reference(row_ptr, uid, val, rows, M, True))


def call(row_ptr, uid, val, shape, **kw):
    W, st = engine.weights_from_pairs(torch.from_numpy(row_ptr), t_u16(uid), t_u16(val), shape, **kw)
    status = engine.PairsStatus.from_tensor(st)  # synchronises
    return W.cpu(), status


SHAPES = [(1, 8), (3, 8), (MANY, 8), (3, 12), (MANY, 12), (3, 264), (MANY, 264), (1, 4096)]


@pytest.mark.parametrize("upscale", [False, True], ids=["raw", "upscale"])
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("rows,M", SHAPES, ids=[f"{r}x{m}" for r, m in SHAPES])
def test_dense_equals_reference(rows, M, offset, upscale):
    row_ptr, uid, val, ref, ref_up = case(rows, M)
    out = None
    if offset:
        buf = torch.full((rows * M + 2 * offset,), 0x5A5A, dtype=torch.int16, device="cuda").view(torch.uint16)
        out = buf[offset:offset + rows * M].view(rows, M)
        assert out.data_ptr() % 16 == 2 * offset
    W, st = call(row_ptr, uid, val, (rows, M), upscale=upscale, out=out)
    assert W.dtype == torch.uint16 and tuple(W.shape) == (rows, M)
    assert torch.equal(W, ref_up if upscale else ref)
    assert (st.dropped, st.conflict_rows, st.bad_rows) == (0, 0, 0)
    if offset:  # the elements either side of the view are untouched
        guard = buf.cpu().view(torch.int16)
        assert int(guard[0]) == 0x5A5A and int(guard[-1]) == 0x5A5A


def test_leading_dimensions_and_no_status():
    row_ptr, uid, val, ref, _ = case(MANY, 12)
    W, st = engine.weights_from_pairs(torch.from_numpy(row_ptr), t_u16(uid), t_u16(val), (5, 2, 103, 12),
                                      want_status=False)
    assert st is None and tuple(W.shape) == (5, 2, 103, 12)
    assert torch.equal(W.cpu().reshape(MANY, 12), ref)
    # device inputs are taken as they are
    dev = [t.cuda() for t in (torch.from_numpy(row_ptr), t_u16(uid), t_u16(val))]
    W2, _ = engine.weights_from_pairs(*dev, (MANY, 12))
    assert torch.equal(W2.cpu(), ref)


def test_zero_rows():
    W, st = engine.weights_from_pairs(torch.zeros(1, dtype=torch.int64), t_u16([]), t_u16([]), (0, 8))
    assert tuple(W.shape) == (0, 8)
    assert engine.PairsStatus.from_tensor(st) == engine.PairsStatus(0, 0, 0)


@pytest.mark.parametrize("M", [12, 264])
@pytest.mark.parametrize("upscale", [False, True], ids=["raw", "upscale"])
def test_dropped_pairs_are_counted_exactly(M, upscale):
    row_ptr, uid, val, _, _ = case(3, M)
    rows = [list(zip(uid[row_ptr[r]:row_ptr[r + 1]].tolist(), val[row_ptr[r]:row_ptr[r + 1]].tolist()))
            for r in range(3)]
    # deregistered uids, among them the row's largest weight: it must not enter rowmax
    rows[0] = [(M, 65535)] + rows[0][:2] + [(65535, 7), (M + 5, 0)] + rows[0][2:]
    rows[2] = rows[2] + [(65535, 65535), (M, 1)]
    planted = 5
    rp, u, v = lists_of(rows)
    W, st = call(rp, u, v, (3, M), upscale=upscale)
    assert st.dropped == planted and st.conflict_rows == 0 and st.bad_rows == 0
    assert torch.equal(W, reference(rp, u, v, 3, M, upscale))


def test_equal_valued_duplicates_are_harmless():
    M = 264
    row_ptr, uid, val, _, _ = case(3, M)
    rows = [list(zip(uid[row_ptr[r]:row_ptr[r + 1]].tolist(), val[row_ptr[r]:row_ptr[r + 1]].tolist()))
            for r in range(3)]
    rows[0] = rows[0] + [rows[0][3], rows[0][150]]   # repeats from the first and the third 64-pair chunk
    rows[1] = [rows[1][-1]] + rows[1]
    rp, u, v = lists_of(rows)
    for upscale in (False, True):
        W, st = call(rp, u, v, (3, M), upscale=upscale)
        assert st.conflict_rows == 0 and st.dropped == 0
        assert torch.equal(W, reference(rp, u, v, 3, M, upscale))


def test_conflicting_duplicates_count_rows_and_keep_one_candidate():
    M = 264
    row_ptr, uid, val, _, _ = case(3, M)
    rows = [list(zip(uid[row_ptr[r]:row_ptr[r + 1]].tolist(), val[row_ptr[r]:row_ptr[r + 1]].tolist()))
            for r in range(3)]
    assert len(rows[0]) == 200 and len(rows[2]) == 65
    # row 0: one uid at positions 5 and 150, in different 64-pair chunks; and a triple in one chunk
    u0, v0 = rows[0][5]
    rows[0][150] = (u0, (v0 + 1000) % 65536)
    u1, v1 = rows[0][70]
    rows[0][71] = (u1, v1 ^ 1)
    rows[0][72] = (u1, v1 ^ 2)
    # row 1: an equal-valued duplicate only
    rows[1][10] = rows[1][20]
    # row 2: the 65th pair repeats the first pair's uid with another weight
    u2, v2 = rows[2][0]
    rows[2][64] = (u2, (v2 + 1) % 65536)
    cand = {(0, u0): {v0, (v0 + 1000) % 65536}, (0, u1): {v1, v1 ^ 1, v1 ^ 2}, (2, u2): {v2, (v2 + 1) % 65536}}
    rp, u, v = lists_of(rows)
    W, st = call(rp, u, v, (3, M))
    assert st.conflict_rows == 2 and st.dropped == 0 and st.bad_rows == 0
    ref = reference(rp, u, v, 3, M)
    got = W.view(torch.int16).to(torch.int64) & 0xFFFF
    exp = ref.view(torch.int16).to(torch.int64) & 0xFFFF
    for (r, c), values in cand.items():
        assert int(got[r, c]) in values, (r, c, int(got[r, c]), values)
        exp[r, c] = got[r, c]
    assert torch.equal(got, exp)
    # upscale judges the raw weights: the same two rows
    _, st = call(rp, u, v, (3, M), upscale=True)
    assert st.conflict_rows == 2


@pytest.mark.parametrize("M", [8, 12])
def test_hostile_row_ptr_is_clamped_inside_the_buffers(M):
    rows, nnz = 8, 40
    rng = np.random.default_rng(77 + M)
    uid = rng.integers(0, M, size=nnz)
    val = rng.integers(1, 65536, size=nnz)
    # negative entries, entries beyond nnz, a decreasing pair, the extremes of int64
    row_ptr = np.array([-5, 3, 10, 7, 55, 20, -(2**63), 2**63 - 1, 30], dtype=np.int64)
    b, e, bad = clamp(row_ptr, nnz)
    assert bad.sum() >= 5 and not bad.all()
    G = 64  # sentinel elements either side of W, inside one device buffer
    buf = torch.full((rows * M + 2 * G,), 0x3C3C, dtype=torch.int16, device="cuda").view(torch.uint16)
    out = buf[G:G + rows * M].view(rows, M)
    # the lists sit inside guarded buffers of their own
    ubuf = torch.full((nnz + 2 * G,), 3, dtype=torch.int16, device="cuda").view(torch.uint16)
    vbuf = torch.full((nnz + 2 * G,), 0x7777, dtype=torch.int16, device="cuda").view(torch.uint16)
    ubuf[G:G + nnz].copy_(t_u16(uid))
    vbuf[G:G + nnz].copy_(t_u16(val))
    W, st = engine.weights_from_pairs(torch.from_numpy(row_ptr), ubuf[G:G + nnz], vbuf[G:G + nnz], (rows, M), out=out)
    status = engine.PairsStatus.from_tensor(st)
    assert status.bad_rows == int(bad.sum()) and status.dropped == 0
    host = buf.cpu().view(torch.int16)
    assert bool((host[:G] == 0x3C3C).all()) and bool((host[G + rows * M:] == 0x3C3C).all())
    ref = reference(row_ptr, uid, val, rows, M).view(torch.int16).to(torch.int64) & 0xFFFF
    got = W.cpu().view(torch.int16).to(torch.int64) & 0xFFFF
    # duplicates inside a clamped range may conflict: such an element holds one of its candidates
    for r in range(rows):
        for c in range(M):
            values = {int(v) for u_, v in zip(uid[b[r]:e[r]], val[b[r]:e[r]]) if u_ == c} or {0}
            assert int(got[r, c]) in values, (r, c)
            if len(values) == 1:
                assert int(got[r, c]) == int(ref[r, c])
    # the value 0x7777 of the list guards never reached W unless a pair holds it
    assert not bool(((got == 0x7777) & (ref != 0x7777)).any())


def test_upscale_ties_small_and_full_maxima_and_zero_rows():
    M = 12
    rows = [
        [(0, 2), (5, 1), (7, 0)],                            # rowmax 2: 1 -> 32767.5 -> 32768
        [(11, 6), (1, 3), (2, 1), (3, 5), (4, 2), (6, 4)],   # rowmax 6: ties at 1, 3 and 5
        [(4, 1)],                                            # rowmax 1
        [(3, 65535), (2, 65534), (9, 1), (0, 32768)],        # rowmax 65535: the identity
        [(1, 0), (2, 0)],                                    # all-zero weights: stays 0
        [],                                                  # no pairs
        [(8, 65534), (0, 32767), (1, 1), (5, 65533)],        # rowmax 65534
        [(2, 3), (12, 9), (65535, 65535)],                   # the larger weights are dropped: rowmax 3
    ]
    rp, u, v = lists_of(rows)
    W, st = call(rp, u, v, (len(rows), M), upscale=True)
    ref = reference(rp, u, v, len(rows), M, upscale=True)
    assert torch.equal(W, ref)
    got = W.numpy().astype(np.int64)
    assert got[0, 5] == 32768 and got[1, 1] == 32768 and got[1, 2] == 10922 and got[1, 3] == 54612
    assert got[2, 4] == 65535 and got[3].tolist()[:4] == [32768, 0, 65534, 65535]
    assert not got[4].any() and not got[5].any() and got[7, 2] == 65535
    assert (st.dropped, st.conflict_rows, st.bad_rows) == (2, 0, 0)


def test_status_words_are_zeroed_by_every_call():
    M = 12
    rows = [[(0, 1), (0, 2), (12, 5)], [(1, 1)], [(3, 4), (3, 5), (40, 1), (41, 1)]]
    rp, u, v = lists_of(rows)
    row_ptr = torch.from_numpy(rp).cuda()
    row_ptr[3] = 99  # one bad row
    uid, val = t_u16(u).cuda(), t_u16(v).cuda()
    W = torch.empty(3, M, dtype=torch.uint16, device="cuda")
    status = torch.full((4,), 0x7F7F7F7F, dtype=torch.int32, device="cuda")
    lib = engine.load_library()
    stream = torch.cuda.current_stream().cuda_stream
    for _ in range(2):
        rc = lib.yuma_weights_from_pairs(3, M, uid.numel(), row_ptr.data_ptr(), uid.data_ptr(), val.data_ptr(), 0,
                                         W.data_ptr(), status.data_ptr(), stream)
        assert rc == 0, lib.yuma_last_error()
        assert status.cpu().tolist() == [3, 2, 1, 0]


def test_graph_replays_follow_the_lists():
    rows, M = MANY, 264
    row_ptr, uid, val, ref, ref_up = case(rows, M)
    rp, u = torch.from_numpy(row_ptr).cuda(), t_u16(uid).cuda()
    v = t_u16(val).cuda()
    for upscale, first in ((False, ref), (True, ref_up)):
        v.copy_(t_u16(val))
        W = torch.empty(rows, M, dtype=torch.uint16, device="cuda")
        engine.weights_from_pairs(rp, u, v, (rows, M), upscale=upscale)  # code objects loaded before the capture
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            _, st = engine.weights_from_pairs(rp, u, v, (rows, M), upscale=upscale, out=W)
        W.view(torch.int16).fill_(0x1111)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(W.cpu(), first)
        assert st.cpu().tolist() == [0, 0, 0, 0]
        # new weights in place, with one uid >= M and one conflict: the replay reads them
        val2 = (val * 7 + 1) % 65536
        uid2 = uid.copy()
        uid2[row_ptr[1]] = M
        uid2[row_ptr[2] + 1] = uid2[row_ptr[2]]
        val2[row_ptr[2] + 1] = (val2[row_ptr[2]] + 1) % 65536
        v.copy_(t_u16(val2))
        u.copy_(t_u16(uid2))
        g.replay()
        torch.cuda.synchronize()
        Wd, std = engine.weights_from_pairs(rp, u, v, (rows, M), upscale=upscale)
        direct = engine.PairsStatus.from_tensor(std)
        assert engine.PairsStatus.from_tensor(st) == direct == engine.PairsStatus(1, 1, 0)
        # (the conflicting element may differ between two runs: it is left out of the comparison)
        a, b = W.cpu().clone().view(torch.int16), Wd.cpu().view(torch.int16)
        c = int(uid2[row_ptr[2]])
        a[2, c] = b[2, c]
        assert torch.equal(a, b)
        exp = reference(row_ptr, uid2, val2, rows, M, upscale).view(torch.int16)
        exp[2, c] = b[2, c]
        assert torch.equal(b, exp)
        u.copy_(t_u16(uid))


def test_end_to_end_pairs_to_run():
    E, N, V, M = 6, 2, 5, 264
    rng = np.random.default_rng(0xE2E)
    w = rng.integers(1, 65536, size=(E, N, V, M), dtype=np.int64)
    w[rng.random(w.shape) < 0.6] = 0
    w[..., 3] = 65535
    W0 = t_u16(w)
    row_ptr, uid, val = engine.pairs_from_dense(W0)
    assert uid.numel() == int((w != 0).sum())
    W1, st = engine.weights_from_pairs(row_ptr, uid, val, (E, N, V, M))
    assert engine.PairsStatus.from_tensor(st) == engine.PairsStatus(0, 0, 0)
    assert torch.equal(W1.cpu(), W0)
    # ... and from the device tensor's own pairs
    rp_d, uid_d, val_d = engine.pairs_from_dense(W1)
    assert torch.equal(rp_d.cpu(), row_ptr) and torch.equal(uid_d.cpu(), uid) and torch.equal(val_d.cpu(), val)
    S = torch.from_numpy(synth.stakes(0xE2E, E, N, V, period=2))
    cfg = YumaConfig(simulation=SimulationHyperparameters(bond_penalty=0.99), yuma_params=YumaParams())
    for variant in (Y3, Y4):
        params = [engine.make_params(variant, cfg)] * N
        a = engine.run(variant, params, W1, S)
        b = engine.run(variant, params, W0, S)
        torch.cuda.synchronize()
        assert a.extra["w_path"] == "u16" and b.extra["w_path"] == "u16"
        for k in ("Dn", "C", "I", "B_final"):
            assert torch.equal(getattr(a, k), getattr(b, k)), k
        assert float(a.Dn.sum()) > 0
