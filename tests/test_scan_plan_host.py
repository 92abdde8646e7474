"""Which bond scan a call reaches (no GPU): yuma_scan_plan's C-ABI and the bond
rows of DESIGN.md section 2.0 as a table. The engine's runs launch what
plan_scan returns; yuma_scan_plan reports the same function's answer, so this
table holds the dispatch to its specification. Every expectation below is
written out by hand from the table and the comments beside the thresholds in
yuma_engine.hip, not computed by a copy of the ladder.

Block geometry used for the grids (rows x miners per block):
  k_bonds       all rows x 64     (grid N * tiles, tiles = ceil(M / 64))
  k_bonds_cn    all rows x 16     (grid N * ceil(M / 16), 512 threads)
  k_rust_big    64 x 64
  wide          4 x 1024          (512 threads)
  tile[_hist]   32 x 64
  flat1 / 2     4 / 8 x 256
  k_bonds_grp   32 x 64, 4 scenarios per block"""

from __future__ import annotations

import ctypes
import os
import re

import pytest

from yuma_simulation._internal import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUST, Y1, Y2, Y3, Y4 = range(5)
EINVAL, EUNSUPPORTED = -1, -4


def header_code():
    text = open(os.path.join(ROOT, "include", "yuma_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_export_and_argtypes_agree():
    code = header_code()
    m = re.search(r"\b(\w+)\s+yuma_scan_plan\s*\((.*?)\)\s*;", code, flags=re.S)
    assert m.group(1) == "int"
    args = [re.sub(r"\s+", " ", a).strip() for a in m.group(2).split(",")]
    assert args == ["int variant", "int N", "int E", "int V", "int M", "const yuma_outputs_t* out",
                    "const yuma_run_options_t* opts", "int vector_form", "int has_sched", "int shard_stage",
                    "yuma_scan_plan_t* plan"]
    assert "yuma_scan_plan" in engine.EXPORTED_SYMBOLS
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    assert list(engine.load_library().yuma_scan_plan.argtypes) == [i32] * 5 + [vp, vp] + [i32] * 3 + [vp]
    # the struct: the header's fields in order, and its enums as engine names them
    body = re.search(r"typedef struct \{([^}]*)\}\s*yuma_scan_plan_t;", code).group(1)
    fields = re.findall(r"\b(?:long long|int32_t)\s+(\w+)\s*;", body)
    assert fields == [name for name, _ in engine.YumaScanPlanC._fields_]
    assert ctypes.sizeof(engine.YumaScanPlanC) == 80
    enum = dict((k, int(v)) for k, v in re.findall(r"\b(YUMA_(?:SCAN|ELEM|DP)_\w+)\s*=\s*(\d+)", code))
    assert [enum[k] for k in ("YUMA_SCAN_TILE", "YUMA_SCAN_STRIP", "YUMA_SCAN_RUST_BIG", "YUMA_SCAN_ELEM",
                              "YUMA_SCAN_GRP")] == [engine.SCAN_FORMS.index(n) for n in
                                                    ("k_bonds", "k_bonds_cn", "k_rust_big", "k_bonds_elem",
                                                     "k_bonds_grp")]
    assert [enum[k] for k in ("YUMA_ELEM_NONE", "YUMA_ELEM_WIDE", "YUMA_ELEM_TILE_HIST", "YUMA_ELEM_TILE",
                              "YUMA_ELEM_FLAT1", "YUMA_ELEM_FLAT2")] == [
        engine.ELEM_SHAPES.index(n) for n in (None, "wide", "tile_hist", "tile", "flat1", "flat2")]
    assert [enum[k] for k in ("YUMA_DP_TV", "YUMA_DP_VQ", "YUMA_DP_QTE")] == [
        engine.DP_LAYOUTS.index(n) for n in ("TV", "VQ", "QTE")]


def row(id, variant, V, M, expect, N=2, **kw):
    return pytest.param(variant, N, V, M, kw, expect, id=id)


def tile(rows, block, grid, **kw):
    return dict(form="k_bonds", shape=None, rows=rows, block=block, grid=grid, rowblocks=1, dpl="TV", rq=False, **kw)


def strip(rows, grid, rq=True, **kw):
    return dict(form="k_bonds_cn", shape=None, rows=rows, block=512, grid=grid, rowblocks=1, dpl="TV", rq=rq, **kw)


def elem(shape, grid, **kw):
    dims = {"wide": (2, 512, "VQ", True), "tile_hist": (2, 256, "TV", True), "tile": (2, 256, "TV", False),
            "flat1": (1, 256, "QTE", False), "flat2": (2, 256, "QTE", False)}[shape]
    return dict(form="k_bonds_elem", shape=shape, rows=dims[0], block=dims[1], dpl=dims[2], nt=dims[3], grid=grid,
                **kw)


H = dict(want_hist=True)
HS = dict(want_hist=True, hist_stride=3)
BF = dict(want_hist=True, hist_bf16=True)
BFS = dict(want_hist=True, hist_bf16=True, hist_stride=3)
SCALAR = dict(vector_form=False)
SHARD = dict(shard_stage=True)

TABLE = [
    # --- bonds, Yuma 0: k_bonds up to 64 validators, the strip scan above (vector form, no W_b / B_inst),
    # rows per lane 1 to 128 validators, 2 to 256, 4 to 512, 8 above; the launch pair above 1024.
    # M = 72: 2 tiles, 5 strips
    row("rust-V16", RUST, 16, 72, tile(1, 256, 4, hist=True, hs=False, ptiles=2), **H),
    row("rust-V17", RUST, 17, 72, tile(4, 256, 4, hist=True, hs=False, ptiles=2, cblocks=2), **H),
    row("rust-V64", RUST, 64, 72, tile(4, 256, 4, hist=True, hs=False, nt=False, ptiles=2, cblocks=2), **H),
    row("rust-V65", RUST, 65, 72, strip(1, 10, hist=True, hs=False, ptiles=5, cblocks=5), **H),
    row("rust-V128", RUST, 128, 72, strip(1, 10, hist=True, hs=False, nt=False, ptiles=5, cblocks=5), **H),
    row("rust-V129", RUST, 129, 72, strip(2, 10, hist=True, hs=False, ptiles=5, cblocks=5), **H),
    row("rust-V256", RUST, 256, 72, strip(2, 10, hist=True, hs=False, ptiles=5, cblocks=5), **H),
    row("rust-V257", RUST, 257, 72, strip(4, 10, hist=True, hs=False, ptiles=5, cblocks=5), **H),
    row("rust-V512", RUST, 512, 72, strip(4, 10, hist=True, hs=False, ptiles=5, cblocks=5), **H),
    row("rust-V513", RUST, 513, 72, strip(8, 10, hist=True, hs=False, ptiles=5, cblocks=5), **H),
    row("rust-V1024", RUST, 1024, 72, strip(8, 10, hist=True, hs=False, ptiles=5, cblocks=5), **H),
    # 1025 validators: 17 row blocks of 64, 2 tiles
    row("rust-V1025", RUST, 1025, 72, dict(form="k_rust_big", shape=None, block=256, rowblocks=17, cblocks=2,
                                           grid=2 * 17 * 2, ptiles=2, dpl="TV"), **H),
    row("rust-V1025-scalar", RUST, 1025, 72, dict(form="k_rust_big", grid=2 * 17 * 2, vector_form=False), **SCALAR),
    row("rust-V65-nohist", RUST, 65, 72, strip(1, 10, hist=False, hs=False)),
    row("rust-V65-strided", RUST, 65, 72, strip(1, 10, hist=True, hs=True), **HS),
    row("rust-V16-strided", RUST, 16, 72, tile(1, 256, 4, hist=True, hs=True), **HS),
    # (no screened reciprocals in a stage)
    row("rust-V65-shard", RUST, 65, 72, strip(1, 10, rq=False, hist=True, hs=False, ptiles=5, cblocks=5), **H, **SHARD),
    # else k_bonds<256, 16> to 256 validators, <1024, 16> above: the scalar form, W_b requested
    row("rust-V65-scalar", RUST, 65, 72, tile(16, 256, 4, hist=True, hs=False, ptiles=2, cblocks=2), **H, **SCALAR),
    row("rust-V256-scalar", RUST, 256, 72, tile(16, 256, 4), **H, **SCALAR),
    row("rust-V257-scalar", RUST, 257, 72, tile(16, 1024, 4, hist=True, hs=False, ptiles=2, cblocks=2), **H, **SCALAR),
    row("rust-V1024-scalar-strided", RUST, 1024, 72, tile(16, 1024, 4, hs=True), **HS, **SCALAR),
    row("rust-V200-Wb", RUST, 200, 72, tile(16, 256, 4, hist=False, hs=False, ptiles=2, cblocks=2), want=("Wb",)),
    row("rust-V300-Binst", RUST, 300, 72, tile(16, 1024, 4), want=("B_inst",)),
    # --- bonds, Yuma 1 / 2: as Yuma 0 without csb; csb (V > 1024, or V > 64 with none of Wn / Wc / T_v /
    # W_b / B_inst requested): k_bonds_elem
    row("yuma1-V16", Y1, 16, 72, tile(1, 256, 4), **H),
    row("yuma2-V64", Y2, 64, 72, tile(4, 256, 4), **H),
    row("yuma1-V65-csb", Y1, 65, 72, elem("tile_hist", 2 * 3 * 2, rq=False, hs=False, ptiles=2), **H),
    row("yuma2-V65-csb-nohist", Y2, 65, 72, elem("flat1", 2 * 17 * 1, rq=True, ptiles=2)),
    row("yuma1-V65-Wn", Y1, 65, 72, strip(1, 10, hist=False, hs=False, ptiles=5, cblocks=5), want=("Wn",)),
    row("yuma2-V300-Tv", Y2, 300, 72, strip(4, 10), want=("Tv",)),
    row("yuma1-V65-Wb", Y1, 65, 72, tile(16, 256, 4), want=("Wb",)),
    row("yuma1-V65-Wn-scalar", Y1, 65, 72, tile(16, 256, 4), want=("Wn",), **SCALAR),
    row("yuma1-V1025-Wb", Y1, 1025, 72, elem("flat1", 2 * 257 * 1, rq=True), want=("Wb",)),
    row("yuma2-V1025-hist", Y2, 1025, 72, elem("tile_hist", 2 * 33 * 2), **H),
    # the wide history scan from 1024 miners, RQ for Yuma 1 / 2 in a run
    row("yuma1-wide", Y1, 70, 1024, elem("wide", 2 * 18 * 1, rq=True, hs=False, hist_bf16=False, ptiles=16), **H),
    row("yuma2-wide-strided", Y2, 70, 1028, elem("wide", 2 * 18 * 2, rq=True, hs=True, ptiles=17), **HS),
    row("yuma1-wide-shard", Y1, 70, 1024, elem("wide", 2 * 18 * 1, rq=False, hist=True, hs=False, ptiles=16, cblocks=1, rowblocks=18), **H, **SHARD),
    row("yuma1-M1020", Y1, 70, 1020, elem("tile_hist", 2 * 3 * 16, rq=False), **H),
    row("yuma1-nohist-shard", Y1, 70, 1024, elem("flat1", 2 * 18 * 4, rq=False), **SHARD),
    row("yuma1-scalar-hist", Y1, 70, 1022, elem("flat1", 2 * 18 * 4, rq=False, hs=False, hist=True), **H, **SCALAR),
    # --- bonds, Yuma 3 / 4: k_bonds_elem at every validator count
    row("yuma3-V16-M64", Y3, 16, 64, elem("tile_hist", 2 * 1 * 1, rq=False, hs=False, hist_bf16=False, ptiles=1), **H),
    row("yuma4-V17-M1020", Y4, 17, 1020, elem("tile_hist", 2 * 1 * 16, rq=False), **H),
    row("yuma3-V65-M1024", Y3, 65, 1024, elem("wide", 2 * 17 * 1, rq=False, hs=False, ptiles=16), **H),
    row("yuma4-V129-M1028", Y4, 129, 1028, elem("wide", 2 * 33 * 2, rq=False, ptiles=17), **H),
    row("yuma3-V1025-M1028", Y3, 1025, 1028, elem("wide", 2 * 257 * 2, rq=False), **H),
    row("yuma3-V1024-M260", Y3, 1024, 260, elem("tile_hist", 2 * 32 * 5, hist=True, hs=False, ptiles=5, cblocks=5, rowblocks=32), **H),
    row("yuma3-V1025-M260", Y3, 1025, 260, elem("tile_hist", 2 * 33 * 5), **H),
    row("yuma3-wide-strided", Y3, 70, 1028, elem("wide", 2 * 18 * 2, hs=True, hist_bf16=False), **HS),
    row("yuma3-wide-bf16", Y3, 70, 1024, elem("wide", 2 * 18 * 1, hs=False, hist_bf16=True, rq=False), **BF),
    row("yuma4-wide-bf16-strided", Y4, 70, 1028, elem("wide", 2 * 18 * 2, hs=True, hist_bf16=True), **BFS),
    row("yuma3-tile-strided", Y3, 70, 1020, elem("tile_hist", 2 * 3 * 16, hs=True, hist_bf16=False), **HS),
    row("yuma4-tile-bf16", Y4, 70, 260, elem("tile_hist", 2 * 3 * 5, hs=False, hist_bf16=True), **BF),
    row("yuma3-tile-bf16-strided", Y3, 70, 1020, elem("tile_hist", 2 * 3 * 16, hs=True, hist_bf16=True), **BFS),
    row("yuma3-Wb-hist", Y3, 70, 260, elem("tile_hist", 2 * 3 * 5), want=("Wb",), **H),
    # without the history: the flat 256 x 256 form, RQ in vector form in a run
    row("yuma3-nohist", Y3, 70, 260, elem("flat1", 2 * 18 * 2, rq=True, hist=False, hs=False, ptiles=5)),
    row("yuma4-nohist-M64", Y4, 256, 64, elem("flat1", 2 * 64 * 1, rq=True)),
    row("yuma3-nohist-shard", Y3, 70, 260, elem("flat1", 2 * 18 * 2, rq=False, hist=False, hs=False, ptiles=5, cblocks=2, rowblocks=18), **SHARD),
    row("yuma3-nohist-Wb", Y3, 70, 260, elem("flat1", 2 * 18 * 2, rq=True), want=("Wb",)),
    # two rows per lane from N * ceil(V / 8) * ceil(M / 256) = 4096 blocks: 63 * 65 = 4095, 64 * 64 = 4096
    row("yuma3-4095", Y3, 504, 16640, elem("flat1", 126 * 65, rq=True), N=1),
    row("yuma3-4096", Y3, 512, 16384, elem("flat2", 64 * 64, rq=True, hist=False, hs=False, ptiles=256, cblocks=64, rowblocks=64), N=1),
    row("yuma3-4095-N5", Y3, 504, 3328, elem("flat1", 5 * 126 * 13, rq=True), N=5),  # 5 * 63 * 13 = 4095
    row("yuma1-4096-N32", Y1, 72, 4096, elem("flat2", 32 * 9 * 16, rq=True), N=32),  # 32 * 9 * 16 = 4608
    row("yuma4-4096-scalar", Y4, 512, 16382, elem("flat2", 64 * 64, rq=False), N=1, **SCALAR),
    # the scalar form writes its history from the flat shapes
    row("yuma3-scalar-hist", Y3, 70, 262, elem("flat1", 18 * 2, rq=False, hist=True, hs=False), N=1, **H, **SCALAR),
    row("yuma3-scalar-strided", Y3, 70, 262, elem("flat1", 18 * 2, rq=False, hist=True, hs=True), N=1, **HS,
        **SCALAR),
    row("yuma4-scalar-strided-4096", Y4, 512, 16382, elem("flat2", 64 * 64, rq=False, hs=True), N=1, **HS, **SCALAR),
    row("yuma3-scalar-wide-M", Y3, 70, 1026, elem("flat1", 2 * 18 * 5, rq=False), **H, **SCALAR),
    # uint16 weights
    row("u16-wide", Y3, 70, 1028, elem("wide", 2 * 18 * 2, w_u16=True, rq=False), w_u16=True, **H),
    row("u16-tile-bf16", Y4, 70, 260, elem("tile_hist", 2 * 3 * 5, w_u16=True, hist_bf16=True), w_u16=True, **BF),
    row("u16-nohist", Y4, 70, 260, elem("flat1", 2 * 18 * 2, w_u16=True, rq=True), w_u16=True),
    # an input schedule: the screened reciprocal without a history, a non-temporal tile history
    row("sched-nohist", Y3, 70, 260, elem("flat1", 2 * 18 * 2, sc=True, rq=True, hist=False), sched=True),
    row("sched-nohist-4096", Y4, 512, 16384, elem("flat2", 64 * 64, sc=True, rq=True), N=1, sched=True),
    row("sched-tile", Y3, 70, 260, elem("tile_hist", 2 * 3 * 5, sc=True, rq=False, hs=False), sched=True, **H),
    row("sched-tile-strided", Y4, 70, 260, elem("tile_hist", 2 * 3 * 5, sc=True, hs=True), sched=True, **HS),
    row("sched-wide", Y4, 70, 1024, elem("wide", 2 * 18 * 1, sc=True, rq=False), sched=True, **H),
    row("sched-wide-bf16-u16", Y3, 70, 1028, elem("wide", 2 * 18 * 2, sc=True, hist_bf16=True, w_u16=True),
        sched=True, w_u16=True, **BF),
    # shared inputs: the sweep scan from 2 scenarios in vector form (groups of 4); else the 64-miner tiles
    row("shared-N1", Y3, 70, 260, elem("tile", 1 * 3 * 5, rq=False, hist=False), N=1, shared_inputs=True),
    row("shared-N1-hist", Y3, 70, 260, elem("tile_hist", 1 * 3 * 5, rq=False, hist=True), N=1, shared_inputs=True, **H),
    row("shared-N2", Y3, 70, 260, dict(form="k_bonds_grp", shape=None, rows=2, block=256, rowblocks=3, cblocks=5,
                                       grid=1 * 3 * 5, hist=False, hs=False, rq=True, dpl="TV", ptiles=5),
        shared_inputs=True),
    row("shared-N6-hist", Y4, 70, 260, dict(form="k_bonds_grp", grid=2 * 3 * 5, hist=True, hs=False, ptiles=5, cblocks=5,
                                            rowblocks=3), N=6,
        shared_inputs=True, **H),
    row("shared-N2-strided", Y4, 70, 260, dict(form="k_bonds_grp", grid=1 * 3 * 5, hist=True, hs=True),
        shared_inputs=True, **HS),
    row("shared-N2-wide", Y3, 70, 1024, elem("wide", 2 * 18 * 1, rq=False), shared_inputs=True, **H),
    row("shared-N2-scalar", Y3, 70, 262, elem("flat1", 2 * 18 * 2, rq=False), shared_inputs=True, **SCALAR),
    row("shared-N2-yuma1", Y1, 70, 260, elem("tile", 2 * 3 * 5, rq=False), shared_inputs=True),
]


@pytest.mark.parametrize("variant,N,V,M,kw,expect", TABLE)
def test_design_table_bond_rows(variant, N, V, M, kw, expect):
    p = engine.scan_plan(variant, N, 8, V, M, **kw)
    got = {k: getattr(p, k) for k in expect}
    assert got == expect, p
    assert p.grid == (p.rowblocks * p.cblocks * (N if p.form != "k_bonds_grp" else (N + 3) // 4))


def test_refusals():
    lib = engine.load_library()
    with pytest.raises(engine.EngineError):  # a bfloat16 history: Yuma 3 / Yuma 4
        engine.scan_plan(Y1, 2, 8, 70, 260, want_hist=True, hist_bf16=True)
    with pytest.raises(engine.EngineError):  # ... in vector form
        engine.scan_plan(Y3, 2, 8, 70, 262, want_hist=True, hist_bf16=True)
    with pytest.raises(engine.EngineError):  # uint16 W: up to 1024 validators
        engine.scan_plan(Y3, 2, 8, 1025, 260, w_u16=True)
    with pytest.raises(engine.EngineError):  # a schedule: no shared inputs
        engine.scan_plan(Y3, 2, 8, 70, 260, sched=True, shared_inputs=True)
    with pytest.raises(engine.EngineError):  # a shard stage takes no schedule
        engine.scan_plan(Y3, 2, 8, 70, 260, sched=True, shard_stage=True)
    outs, p = engine.YumaOutputsC(), engine.YumaScanPlanC()
    args = (ctypes.addressof(outs), None, 1, 0, 0)
    assert lib.yuma_scan_plan(5, 2, 8, 70, 260, *args, ctypes.addressof(p)) == EINVAL
    assert lib.yuma_scan_plan(Y3, 2, 8, 0, 260, *args, ctypes.addressof(p)) == EINVAL
    assert lib.yuma_scan_plan(Y3, 2, 8, 70, 260, *args, None) == EINVAL
    assert lib.yuma_scan_plan(Y3, 2, 8, 70, 260, None, None, 1, 0, 0, ctypes.addressof(p)) == EINVAL
    assert lib.yuma_scan_plan(Y3, 2, 8, 70, 260, *args, ctypes.addressof(p)) == 0


# ---------------------------------------------------------------------------
# The GPU test files name, on each case, the scan the case is there to reach:
# it must reach it, and each list must keep covering what it covers.
# ---------------------------------------------------------------------------
def reached(p):
    """A plan as the case lists spell it: the kernel (k_bonds by block and rows,
    k_bonds_cn by rows per lane) or k_bonds_elem's shape, then its flags."""
    name = {"k_bonds": f"k_bonds<{p.block},{p.rows}>", "k_bonds_cn": f"k_bonds_cn<{p.rows}>",
            "k_bonds_elem": p.shape}.get(p.form, p.form)
    flags = [f for f, on in (("rq", p.rq), ("hs", p.hs), ("bf16", p.hist_bf16), ("sc", p.sc), ("u16", p.w_u16),
                             ("hist", p.form == "k_bonds_grp" and p.hist)) if on]
    return "+".join([name] + flags) + ("" if p.vector_form else "/scalar")


def kernel_of(reach):
    return reach.split("/")[0].split("+")[0]


def check_cases(module, cases):
    got = {}
    for case in cases:
        assert case.reach, case.id
        args, kw = module.plan_args(case)
        got[case.id] = reached(engine.scan_plan(*args, **kw))
    assert got == {case.id: case.reach for case in cases}
    assert {kernel_of(case.reach) for case in cases} == module.COVERED


def test_resume_cases_reach_what_they_name():
    import test_gpu_resume as t

    check_cases(t, t.CASES)
    shards = [c for c in t.CASES if c.kind == "shards"]
    assert {c.id for c in shards} == set(t.SHARDS_RUN_REACH)
    for case in shards:
        args, kw = t.plan_args(case, shard=False)
        assert reached(engine.scan_plan(*args, **kw)) == t.SHARDS_RUN_REACH[case.id], case.id


def test_hist_stride_cases_reach_what_they_name():
    import test_gpu_hist_stride as t

    check_cases(t, t.CASES)
    assert all("+hs" in c.reach for c in t.CASES)  # (the launch pair: its host countdown)


def test_hist_bf16_cases_reach_what_they_name():
    import test_gpu_hist_bf16 as t

    check_cases(t, t.NATIVE)
    for case in t.NATIVE:
        if case.strided:
            args, kw = t.plan_args(case, strided=True)
            assert reached(engine.scan_plan(*args, **kw)) == case.reach.replace("+bf16", "+hs+bf16"), case.id
    assert {kernel_of(c.reach) for c in t.NATIVE if c.strided} == t.COVERED  # both shapes under a stride too
    for case in t.FALLBACK:  # no native bfloat16 history: the engine refuses the plan as it refuses the run
        args, kw = t.plan_args(case)
        with pytest.raises(engine.EngineError):
            engine.scan_plan(*args, **{**kw, "vector_form": case.M % 4 == 0})


def test_sched_shapes_reach_what_they_name():
    import test_gpu_sched as t

    for (shape, hist), reach in t.REACH.items():
        for variant, _ in t.VARIANTS.values():
            args, kw = t.plan_args(shape, hist, variant)
            assert reached(engine.scan_plan(*args, **kw)) == reach, (shape, hist, variant)
    assert {kernel_of(r) for r in t.REACH.values()} == t.COVERED
    # every (shape, history) the tests run is named
    assert set(t.REACH) == {(s, h) for s in ("tile", "wide", "bigv") for h in (True, False)} | {("tworow", False)}
