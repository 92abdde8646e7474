"""Patch sets for tools/ab_build.py: PATCHES[name] = [(old, new[, count]), ...]
applied to yuma-simulation_amd/csrc/yuma_engine.hip. Timing-only builds are
named diag_* (wrong results by design; never used for parity)."""

PATCHES = {
    # k_consensus_w: W loads + division only, no prerank / search (round 3,
    # profiles/r03/ab/consensus_lds_stage_diag.txt "d1")
    "diag_cons_loadonly": [(
        "  const LdsRows s{&rl[0][0], L.wave * 48 * R + 16 * R + L.rg};\n  if (Pout",
        "  const LdsRows s{&rl[0][0], L.wave * 48 * R + 16 * R + L.rg};\n"
        "  {\n    float t = 0.0f;\n    for (int i = 0; i < R; ++i) for (int c = 0; c < 4; ++c) t = t + wn[i][c];\n"
        "    if (t == 1234.5f) craw[slice * M + m] = t;\n    return;\n  }\n  if (Pout")],
    # k_bonds_elem without the dividend-partial stores (profiles/r03/ab/scan_partials_diag.txt)
    "diag_no_dp": [(
        "        d = wsum16(d);  // sum_row16's xor-butterfly tree, on DPP\n        if",
        "        d = wsum16(d);  // sum_row16's xor-butterfly tree, on DPP\n        if (d == 1.2345e-37f)\n        if")],
}

# k_bonds_grp (c3 sweep scan): one scenario per block, four rows per lane
# (the two file-scope constants size the grid in plan_scan as well as the kernel: host dispatch follows the patch)
PATCHES["grp_k1_r4_w4"] = [("constexpr int kScanGroup = 4;", "constexpr int kScanGroup = 1;"),
                           ("constexpr int kGrpRows = 2;", "constexpr int kGrpRows = 4;")]

# k_bonds_elem: settle every pre-loop load (bond state, ring prefetch) before the
# epoch loop, so the waitcnt pass need not drain the ring in the loop
_ELEM_PRE = """#pragma unroll
  for (int k = 0; k < P; ++k)
    if (A.t0 + k < A.t1) fetch(k, A.t0 + k, sched_at<SC>(A, A.t0 + k));
  int snext = sched_at<SC>(A, A.t0 + P);  // SC: the slice of the next epoch to fetch

  for (int tb = A.t0; tb < A.t1; tb += P) {"""
PATCHES["elem_wait0"] = [(_ELEM_PRE, _ELEM_PRE.replace("\n\n  for (int tb", "\n  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)\n\n  for (int tb"))]
# paired consensus at 2 / 5 waves per SIMD
PATCHES["cp_lb2"] = [("__global__ __launch_bounds__(256, 3) void k_consensus_p(", "__global__ __launch_bounds__(256, 2) void k_consensus_p(")]
PATCHES["cp_lb5"] = [("__global__ __launch_bounds__(256, 3) void k_consensus_p(", "__global__ __launch_bounds__(256, 5) void k_consensus_p(")]

# round 5: Yuma / Yuma2 on the wide element-wise history scan (k_bonds_elem
# with the rank pass's column sums): ring depth
PATCHES["cn_p3"] = [("constexpr int kWidePCn = 2;", "constexpr int kWidePCn = 3;")]
PATCHES["cn_p4"] = [("constexpr int kWidePCn = 2;", "constexpr int kWidePCn = 4;")]
# ... and at 4 (128 VGPRs: spills)
PATCHES["cons_w4"] = [("__global__ __launch_bounds__(256, 3) void k_consensus_p(", "__global__ __launch_bounds__(256, 4) void k_consensus_p(")]
# (scan_rowvec / kScanRowUniform: wave-uniform scalar row-sum / stake loads in
# the one-row-per-wave scans, c4 bonds 1.377-1.391 against 1.395-1.402 with
# vector loads: rejected and removed, profiles/r05/ab_c4_rowuniform.txt)

# round 5: the plain streaming rank (k_rank_s, c2 Yuma 3): batch depth and
# non-temporal loads
PATCHES["rank_b4"] = [("  constexpr int B = 8;\n  for (int r0 = L.g; r0 < V; r0 += 16 * B) {",
                       "  constexpr int B = 4;\n  for (int r0 = L.g; r0 < V; r0 += 16 * B) {")]
PATCHES["rank_b16"] = [("  constexpr int B = 8;\n  for (int r0 = L.g; r0 < V; r0 += 16 * B) {",
                        "  constexpr int B = 16;\n  for (int r0 = L.g; r0 < V; r0 += 16 * B) {")]
PATCHES["rank_nt"] = [("      const int rr = min(r0 + 16 * i, V - 1);\n      load4c<VEC>(Ws, rr, V, m, M, w[i]);",
                       "      const int rr = min(r0 + 16 * i, V - 1);\n      load4c<VEC, true>(Ws, rr, V, m, M, w[i]);")]

# sweep scan: 16 epochs of dividend partials parked per flush
PATCHES["grp_db16"] = [("constexpr int kGrpDB = 32;", "constexpr int kGrpDB = 16;")]

# (round 5, rejected and removed: hist_qte, the wide history scan parking its
# quad partials in LDS as the history-less scan does: c2 Yuma 3 bonds 1.560/1.535 -> 1.552/1.549, finalize + k_dte_sum
# 0.008 -> 0.013-0.015 ms; Yuma 1 bonds 1.765 -> 1.74: a wash, rejected,
# profiles/r05/ab_hist_qte.txt)

# (round 5, rejected and removed: YumaRust's strip scan with 2 / 4 waves per
# 16-miner strip block at 256 validators: bonds 3.50 -> 9.12 / 5.11 ms,
# profiles/r05/ab_cn_waves.txt)
# Yuma / Yuma2 wide history scan without k_rowsum's screened reciprocal (per-row IEEE 1/rs + per-element guard)
PATCHES["elem_norq"] = [("constexpr bool kElemRq(int variant, bool hist) { return hist ? variant <= YUMA_VARIANT_YUMA2 : true; }",
                          "constexpr bool kElemRq(int variant, bool hist) { return false; }"),
                         ("constexpr int kNoHistP2 = 2;", "constexpr int kNoHistP2 = 3;")]
# ... and every elem scan (Yuma 3 / 4 history, the history-less c4 / c2 forms): rejected,
# c2 Yuma 3 bonds 1.58 -> 1.80 ms, c4 1.34 -> 1.65 (profiles/r05/ab_elem_rq.txt)
PATCHES["elem_rq_all"] = [("constexpr bool kElemRq(int variant, bool hist) { return hist ? variant <= YUMA_VARIANT_YUMA2 : true; }",
                           "constexpr bool kElemRq(int variant, bool hist) { return true; }")]
# (round 5, rejected and removed: graph captures issuing the input-only phases
# of each of 4 / 8 / 16 pieces on a side stream, so consensus / rank of piece
# k + 1 ran beside the bond scan of piece k: c2 3.80 -> 3.88 / 3.98 / 4.27 ms,
# c3 7.83 -> 8.42, c4 +- 0; profiles/r05/ab_pipeline.txt)
# k_consensus_p timing-only builds (round 5): no histogram atomics / return
# after the load + division (results wrong by design)
PATCHES["diag_consp_noatomic"] = [(
    "          atomicAdd(hp + (col + c) * kHS + (k < w[c] ? k : w[c]), su);",
    "          if (su == 0x7FFFFFFFu) atomicAdd(hp + (col + c) * kHS + (k < w[c] ? k : w[c]), su);")]
PATCHES["diag_consp_loadonly"] = [(
    "  const int col = cq * 4;  // this lane's first column within the pair's 32\n",
    "  const int col = cq * 4;  // this lane's first column within the pair's 32\n"
    "  {\n    float t = 0.0f;\n    for (int i = 0; i < R; ++i) for (int c = 0; c < 4; ++c) t = t + wn[i][c];\n"
    "    if (t == 1234.5f) craw[slice * M + m] = t;\n    return;\n  }\n")]
# (round 5, rejected and removed: k_consensus_pf, a persistent form of
# k_consensus_p at 2 blocks / CU issuing the next tile's W rows (4 / 8 / 12 /
# 16 of 16 per lane) before each search: consensus 0.85 -> 1.02 / 1.05 /
# 1.19 / 1.30 ms; the search needs the third wave per SIMD more than the
# loads need the lead; profiles/r05/ab_consensus_pf.txt)
# (round 5, rejected and removed: k_consensus_p's histogram widened from 64
# to 96 / 128 grid points, so c2's brackets (<= 65 points) finish without a
# bisection pass: consensus 0.85 -> 0.855 / 0.87-0.88; profiles/r05/ab_hist_bins.txt)
# (round 5: the first history-less form loaded {row sum, reciprocal, stake} as
# one 16-byte rq4 record; the compiler copied the reciprocal out of the load's
# register tuple right after issuing it and waited vmcnt(0) each epoch: c4
# bonds 1.25 -> 1.58. The reciprocal is now its own 4-byte load.)
# element-wise scan: unconditional clamped ring refill alone (round 5: c2 1.54 -> 1.56, c4 1.27 -> 1.41, rejected)
PATCHES["elem_refill_clamped"] = [("      if (t + P < A.t1) {\n        fetch(k, t + P, snext);\n        if constexpr (SC) snext = sched_at<SC>(A, t + P + 1);",
                                   "      {\n        fetch(k, min(t + P, A.t1 - 1), snext);\n        if constexpr (SC) snext = sched_at<SC>(A, t + P + 1);")]

# ---------------------------------------------------------------------------
# Round 6: YumaRust's strip scan k_bonds_cn. Timing-only
# builds on top of the LDS-parked dividend partials:
#   diag_cn_nobar   the state-dependent column sum of B_ema from the wave's own
#                   16 rows only (no LDS hand-off, no block barrier)
#   diag_cn_noflush partials parked but never written
PATCHES["diag_cn_nobar"] = [("        cn_wave_sums<NW>(ema, red[par], cq, rr, wave);",
                             "        cn_wave_sums<1>(ema, red[par], cq, rr, wave);")]
PATCHES["diag_cn_noflush"] = [("      if (t - tq == DB - 1 || t == A.t1 - 1) flush_d(t);  // block-uniform",
                               "      if (t - tq == DB - 1 || t == A.t1 - 1) tq = t + 1;")]

# k_bonds_cn ring loads without phis (round 6): bond_alpha loaded from I when
# the scenario is not liquid (no conditional load), and the refills clamped
# to the last epoch instead of skipped
_CN_BA = [("    if (liquid) load4c<true>(A.ba + slice * M, 0, 1, m, M, rba[k]);\n    if (RUST) load4c<true>(A.R + slice * M, 0, 1, m, M, rrk[k]);",
           "    load4c<true>((liquid ? A.ba : A.I) + slice * M, 0, 1, m, M, rba[k]);\n    if (RUST) load4c<true>(A.R + slice * M, 0, 1, m, M, rrk[k]);")]
_CN_CLAMP = [("  for (int k = 0; k < P; ++k)\n    if (A.t0 + k < A.t1) fetch(k, A.t0 + k);\n\n  // RN(1 / d[c])",
              "  for (int k = 0; k < P; ++k) fetch(k, min(A.t0 + k, A.t1 - 1));\n\n  // RN(1 / d[c])"),
             ("      if (t + P < A.t1) fetch(k, t + P);  // slot k consumed: refill it\n      if constexpr (!RUST) {\n        cn_wave_sums<NW>(csum, red[par], cq, rr, wave);",
              "      fetch(k, min(t + P, A.t1 - 1));  // slot k consumed: refill it\n      if constexpr (!RUST) {\n        cn_wave_sums<NW>(csum, red[par], cq, rr, wave);")]
PATCHES["cnl_ba"] = _CN_BA
PATCHES["cnl_clamp"] = _CN_BA + _CN_CLAMP
_CN_P = "constexpr int cn_epochs(int R) { return R <= 2 ? 4 : (R == 4 ? 2 : 1); }"
PATCHES["cnl_p2"] = [(_CN_P, _CN_P.replace("R <= 2 ? 4 :", "R <= 2 ? 2 :"))]
PATCHES["cnl_p3"] = [(_CN_P, _CN_P.replace("R <= 2 ? 4 :", "R <= 2 ? 3 :"))]
PATCHES["cnl_clamp_p3"] = PATCHES["cnl_clamp"] + PATCHES["cnl_p3"]

# k_consensus_p: the pair-shared histogram's bins rotated by 32 for the column
# groups cq >= 4 (lanes cq and cq + 4 hit the same banks at kHS = 68 words)
PATCHES["cp_swz"] = [
    ("          atomicAdd(hp + (col + c) * kHS + (k < w[c] ? k : w[c]), su);",
     "          atomicAdd(hp + (col + c) * kHS + (((k < w[c] ? k : w[c]) + ((cq & 4) << 3)) & 63), su);"),
    ("        const unsigned* hc = hp + (col + c) * kHS + 8 * rg;",
     "        const unsigned* hc = hp + (col + c) * kHS + ((8 * rg + ((cq & 4) << 3)) & 63);")]


# k_consensus_p: two copies of the pair's histogram, lanes of even / odd rg
# adding to their own (same-address atomics of a column's rows halve); the
# readout adds the copies (integers: exact in any order)
PATCHES["cp_hist2"] = [
    ("  __shared__ __attribute__((aligned(16))) unsigned hb[NP * 32 * kHS];  // per pair: 32 columns",
     "  __shared__ __attribute__((aligned(16))) unsigned hb[NP * 2 * 32 * kHS];  // per pair: 32 columns, 2 copies"),
    ("      uint4* hz = reinterpret_cast<uint4*>(hb + pair * 32 * kHS);\n      constexpr int NW4 = 32 * kHS / 4;",
     "      uint4* hz = reinterpret_cast<uint4*>(hb + pair * 2 * 32 * kHS);\n      constexpr int NW4 = 2 * 32 * kHS / 4;"),
    ("      unsigned* hp = hb + pair * 32 * kHS;  // zeroed before the bracket barrier",
     "      unsigned* hp = hb + pair * 2 * 32 * kHS;  // zeroed before the bracket barrier"),
    ("          atomicAdd(hp + (col + c) * kHS + (k < w[c] ? k : w[c]), su);",
     "          atomicAdd(hp + (rg & 1) * 32 * kHS + (col + c) * kHS + (k < w[c] ? k : w[c]), su);"),
    ("        const uint4 a = *reinterpret_cast<const uint4*>(hc);\n        const uint4 b = *reinterpret_cast<const uint4*>(hc + 4);",
     "        const uint4 a0 = *reinterpret_cast<const uint4*>(hc), a1 = *reinterpret_cast<const uint4*>(hc + 32 * kHS);\n"
     "        const uint4 b0 = *reinterpret_cast<const uint4*>(hc + 4), b1 = *reinterpret_cast<const uint4*>(hc + 4 + 32 * kHS);\n"
     "        const uint4 a = make_uint4(a0.x + a1.x, a0.y + a1.y, a0.z + a1.z, a0.w + a1.w);\n"
     "        const uint4 b = make_uint4(b0.x + b1.x, b0.y + b1.y, b0.z + b1.z, b0.w + b1.w);")]
