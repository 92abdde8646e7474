/*
 * yuma_hip.h — C-ABI of libyuma_hip.so, the MI355X (gfx950) engine for the
 * Yuma consensus epoch step of yuma_simulation.
 *
 * The reference has no FFI: its seam is the Python functions
 *   YumaRust/Yuma/Yuma2/Yuma3/Yuma4(W, S, B_old, config)
 *       src/yuma_simulation/_internal/yumas.py:61,175,285,399,494
 * and the epoch loop that threads the bond state through them
 *   run_simulation(case, yuma_version, yuma_config)
 *       src/yuma_simulation/_internal/simulation_utils.py:26-112
 * The entry points below replace exactly those two seams:
 *   yuma_epoch  <- one call of a Yuma* variant (E = 1, every output optional)
 *   yuma_run    <- the whole epoch loop of run_simulation (E epochs, N scenarios)
 * Every run is one yuma_request_t (below) given to yuma_run_request or
 * yuma_graph_create_request; the positional entry points are shims that fill
 * that record from their arguments.
 * The Python mirror (yuma_simulation/_internal/engine.py) binds them with
 * ctypes; INTEGRATION.md shows the binding a maintainer adds to the reference.
 *
 * Conventions
 *  - Every pointer argument is DEVICE memory (hipMalloc / torch.cuda tensors),
 *    fp32 row-major (W alone may be uint16 row-major: YUMA_RUN_W_U16 below),
 *    owned by the caller. The engine never allocates, never
 *    synchronises, and is stream-ordered on `stream` (a hipStream_t, NULL =
 *    default stream), so a call can be captured into a hipGraph.
 *  - Layouts: W [E][N][V][M]; S [E][N][V]; B [N][V][M]; per-epoch vectors
 *    [E][N][V] or [E][N][M]; per-epoch matrices [E][N][V][M].
 *  - Return value: 0 on success, a negative YUMA_E* code otherwise;
 *    yuma_last_error() describes the last failure (thread-local).
 */
#ifndef YUMA_HIP_H
#define YUMA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Variant selector (yumas.py:61 YumaRust, :175 Yuma, :285 Yuma2, :399 Yuma3, :494 Yuma4). */
enum yuma_variant {
  YUMA_VARIANT_RUST = 0,
  YUMA_VARIANT_YUMA1 = 1,
  YUMA_VARIANT_YUMA2 = 2,
  YUMA_VARIANT_YUMA3 = 3,
  YUMA_VARIANT_YUMA4 = 4
};

/* Bond-reset rule applied by run_simulation before an epoch
 * (simulation_utils.py:62-88): Yuma 3.1 resets unconditionally at
 * reset_bonds_epoch; Yuma 3.2 / Yuma 4 only if the previous epoch's
 * consensus of the reset miner is exactly 0. */
enum yuma_reset_mode {
  YUMA_RESET_NONE = 0,
  YUMA_RESET_ALWAYS = 1,
  YUMA_RESET_IF_ZERO_CONSENSUS = 2
};

/* Liquid-alpha modes (yumas.py:231-253 and copies). */
enum yuma_liquid_mode {
  YUMA_LIQUID_OFF = 0,      /* scalar bond_alpha                                 */
  YUMA_LIQUID_QUANTILE = 1, /* consensus high/low from quantiles (or one override) */
  YUMA_LIQUID_CONST_AB = 2  /* both overrides given and unequal: a,b host doubles */
};

enum yuma_override_flags { YUMA_OVR_HIGH = 1, YUMA_OVR_LOW = 2, YUMA_OVR_FORCE_Q99 = 4 };

/* yuma_params_t.flags. YUMA_FLAG_NO_HIST: run the consensus search as the
 * plain bisection even where the exact-stake histogram finish applies (both
 * give the same result; tests compare them). YUMA_FLAG_RESET_ALL_COLUMNS: the
 * reset zeroes every miner column (reset_index ignored) -- the reference's
 * `B_state[:, None] = 0.0` when reset_bonds_index is None
 * (simulation_utils.py:63-64). */
enum yuma_flags { YUMA_FLAG_NO_HIST = 1, YUMA_FLAG_RESET_ALL_COLUMNS = 2 };

/* Per-scenario parameters: the flattened YumaConfig (yumas.py:7-45) with every
 * Python-double constant pre-rounded exactly as the reference's torch ops round
 * them (python scalars meet fp32 tensors as fp32). 128 bytes, naturally aligned. */
typedef struct yuma_params {
  int32_t variant;          /* yuma_variant (must equal the call's variant)        */
  int32_t bisect_iters;     /* trip count of `while (hi-lo) > 1/consensus_precision` */
  int32_t liquid_mode;      /* yuma_liquid_mode                                    */
  int32_t override_flags;   /* yuma_override_flags                                 */
  int32_t reset_mode;       /* yuma_reset_mode                                     */
  int32_t reset_epoch;      /* epoch index of the reset (run_simulation epoch)     */
  int32_t reset_index;      /* miner column to reset, 0 <= reset_index < M         */
  int32_t flags;            /* yuma_flags                                          */
  float kappa;              /* fp32(kappa)                                         */
  float bond_penalty;       /* fp32(beta)                                          */
  float one_minus_bond_penalty; /* fp32(1 - beta), difference taken in double      */
  float bond_alpha;         /* fp32(bond_alpha)                                    */
  float one_minus_bond_alpha;   /* fp32(1 - bond_alpha), difference in double      */
  float alpha_low;          /* fp32(alpha_low)                                     */
  float alpha_high;         /* fp32(alpha_high)                                    */
  float capacity_alpha;     /* fp32(capacity_alpha)           (Yuma3)              */
  float decay_keep;         /* fp32(1 - decay_rate)           (Yuma3)              */
  float maxint;             /* fp32(maxint) = 2^64 for the default (Yuma3)         */
  float const_a;            /* LIQUID_CONST_AB: fp32(a)                            */
  float const_b;            /* LIQUID_CONST_AB: fp32(b)                            */
  double ln_num;            /* log(1/alpha_high-1) - log(1/alpha_low-1)             */
  double ln_low;            /* log(1/alpha_low-1)                                  */
  double override_high;     /* override_consensus_high (if flagged)                */
  double override_low;      /* override_consensus_low (if flagged)                 */
  double reserved1[2];
} yuma_params_t;

/* Optional outputs; any pointer may be NULL (not produced). The dict keys of
 * the reference (yumas.py:264-282 etc.) are noted per field. */
typedef struct yuma_outputs {
  float* Dn;         /* [E][N][V] validator_reward_normalized                    */
  float* D;          /* [E][N][V] validator_reward                               */
  float* C;          /* [E][N][M] server_consensus_weight (quantised)            */
  float* I;          /* [E][N][M] server_incentive                               */
  float* R;          /* [E][N][M] server_rank                                    */
  float* P;          /* [E][N][M] server_prerank                                 */
  float* T;          /* [E][N][M] server_trust                                   */
  float* Tv;         /* [E][N][V] validator_trust                                */
  float* Sn;         /* [E][N][V] stake (normalised)                             */
  float* bond_alpha; /* [E][N][M] liquid bond_alpha per miner (liquid only)      */
  float* alpha_ab;   /* [E][N][2] alpha_a, alpha_b (liquid only)                 */
  float* Wn;         /* [E][N][V][M] weight (row-normalised)                     */
  float* Wc;         /* [E][N][V][M] consensus_clipped_weight                    */
  float* Wb;         /* [E][N][V][M] weight_for_bond (Yuma1/Yuma2)               */
  float* B_inst;     /* [E][N][V][M] validator_bond (Rust/Yuma1/Yuma2)           */
  float* B_hist;     /* [E][N][V][M] bond state after each epoch (bonds_per_epoch);
                        [n_hist][N][V][M] under a history stride (yuma_run_opts);
                        bfloat16 elements under YUMA_RUN_HIST_BF16                 */
  float* B_final;    /* [N][V][M]    bond state after the last epoch             */
} yuma_outputs_t;

enum {
  YUMA_OK = 0,
  YUMA_EINVAL = -1,    /* bad sizes / pointers / params                          */
  YUMA_EWORKSPACE = -2,/* workspace too small                                    */
  YUMA_EHIP = -3,      /* a HIP launch failed                                    */
  YUMA_EUNSUPPORTED = -4
};

/* Validators per slice. Up to YUMA_REG_VALIDATORS a workgroup holds a miner
 * column's validators in registers (the fast paths); above, the engine streams
 * the column from memory in every consensus pass and runs YumaRust's bond
 * normalisation as two launches per epoch (correct at any size up to
 * YUMA_MAX_VALIDATORS, built for the occasional very wide validator set). */
#define YUMA_REG_VALIDATORS 1024
#define YUMA_MAX_VALIDATORS (1 << 20)

/* Bytes of device workspace yuma_run / yuma_epoch need for these sizes.
 * full_outputs != 0 reserves the partial sums the validator_trust output
 * (yuma_outputs_t.Tv) needs; without it a non-NULL Tv is rejected.        */
size_t yuma_workspace_bytes(int variant, int N, int E, int V, int M, int full_outputs);

/* The whole epoch loop of run_simulation (simulation_utils.py:44-110) for N
 * independent scenarios of one variant, E epochs each.
 *   params_dev : [N] yuma_params_t in device memory
 *   W          : [E][N][V][M] raw weights (row-normalised inside, yumas.py:186)
 *   S          : [E][N][V] raw stakes (normalised inside, yumas.py:189)
 *   B_init     : [N][V][M] bond state before epoch 0, or NULL (= B_state None)
 *   Wprev_init : Yuma2 only: [N][V][M] normalised W_prev for epoch 0, or NULL
 *   chunk_epochs: epochs per phase-1 batch (0 = engine default)                */
int yuma_run(int variant, const yuma_params_t* params_dev, int N, int E, int V, int M,
             const float* W, const float* S, const float* B_init, const float* Wprev_init,
             const yuma_outputs_t* out, void* workspace, size_t workspace_bytes,
             int chunk_epochs, void* stream);

/* yuma_run with options. flags: YUMA_RUN_SHARED_INPUTS — every scenario reads
 * the same input trajectory: W is [E][V][M] and S [E][V] (a parameter sweep
 * over one subnet; SURVEY config c3), so a whole sweep moves one copy of W
 * per epoch through HBM and the scenarios' reads of it meet in the caches.
 * Results are those of yuma_run on W and S replicated per scenario.
 * phase_ms: NULL, or per-phase device time as yuma_run_profiled (blocks).
 * YUMA_RUN_W_U16 — W addresses uint16_t elements in the same [E][N][V][M]
 * layout (the on-chain weight format); element w is the weight (float)w, an
 * exact conversion, so every output has the bits of the same run on the
 * widened fp32 tensor, for half the device memory and half the bytes per pass
 * over W. S, params, B_init, Wprev_init, the outputs and the workspace size
 * keep their meaning. W must be 8-byte aligned (and the fp32 matrices 16-byte
 * aligned). Accepted by yuma_run_ex and yuma_graph_create_ex where
 * yuma_u16_native() returns 1; elsewhere they return YUMA_EUNSUPPORTED before
 * the first launch and the caller widens W itself. Every other entry point
 * reads fp32 weights only.
 * YUMA_RUN_HIST_BF16 — out->B_hist addresses bfloat16 elements (2 bytes: the
 * upper half of an fp32) in the same [E or n_hist][N][V][M] layout, written
 * by the bond scan itself: element = RNE(fp32 bond state) for every finite
 * value (a value above the largest finite bfloat16 rounds to infinity, as RNE
 * has it); a NaN stays a NaN, payload unspecified. bfloat16 keeps fp32's
 * exponent range, which Yuma 3's bonds (scaled by maxint = 2^64) need. The
 * history is never fed back into the recurrence: Dn, C, I, B_final and every
 * other output have the bits of the fp32-history run, for half the history's
 * memory and write traffic. A bfloat16 history is for reading, not for
 * resuming: resume from B_final (fp32). B_hist must be non-NULL
 * (YUMA_EINVAL) and 8-byte aligned. Accepted by yuma_run_ex, yuma_run_opts,
 * yuma_graph_create_ex and yuma_graph_create_opts where
 * yuma_hist_bf16_native() returns 1; elsewhere they return YUMA_EUNSUPPORTED
 * before the first launch and the caller converts an fp32 history itself.
 * Combines with YUMA_RUN_W_U16 and with the history stride. yuma_epoch,
 * yuma_run, yuma_run_profiled, yuma_graph_create and yuma_shard_stage write an
 * fp32 history only.                                                         */
enum yuma_run_flags { YUMA_RUN_SHARED_INPUTS = 1, YUMA_RUN_W_U16 = 2, YUMA_RUN_HIST_BF16 = 4 };
int yuma_run_ex(int variant, const yuma_params_t* params_dev, int N, int E, int V, int M,
                const float* W, const float* S, const float* B_init, const float* Wprev_init,
                const yuma_outputs_t* out, void* workspace, size_t workspace_bytes,
                int chunk_epochs, int flags, void* stream, float* phase_ms);

/* yuma_run_ex with an options record: its flags, and a stride for the bond
 * history. With hist_stride = s (0 counts as 1) and hist_first = f the run
 * stores the bond state after the epochs t_j = f + j*s < E only, counted from
 * the run's epoch 0 whatever chunk_epochs is: out->B_hist is
 * [n_hist][N][V][M] with n_hist = yuma_hist_slots(E, s, f), and slot j holds
 * the bits the dense history holds at epoch t_j (resets applied as there).
 * Every other output, B_final included, is that of the dense run. f lets a run
 * resumed from B_final keep the phase of the run it continues. s <= 1 with
 * f = 0 is the dense history on yuma_run_ex's own path. f >= E stores nothing.
 * The history costs n_hist / E of the dense history's memory and write
 * traffic; the stored epochs still go out as whole 16-byte row-contiguous
 * stores, the others skip the store on a block-uniform test of the epoch. On
 * MI355X at 256 x 4096, 1000 epochs, the dense history is 4.19 GB of the bond
 * scan's 8.5 GB of traffic (measured effect: README.md, profiles/hist_stride/).
 * Combines with YUMA_RUN_SHARED_INPUTS, YUMA_RUN_W_U16 and
 * YUMA_RUN_HIST_BF16 as the dense history does. opts NULL: every default. hist_stride < 0, hist_first < 0, an
 * unknown flag or a non-zero reserved word return YUMA_EINVAL before the first
 * launch. The workspace size does not depend on the options.
 * yuma_epoch and yuma_shard_stage (the wide-subnet path) keep the dense
 * history only.                                                              */
typedef struct yuma_run_options {
  int32_t flags;        /* yuma_run_flags                                       */
  int32_t hist_stride;  /* 0 or 1: every epoch                                  */
  int32_t hist_first;   /* first stored epoch                                   */
  int32_t reserved[5];  /* must be 0                                            */
} yuma_run_options_t;   /* 32 bytes */
int yuma_run_opts(int variant, const yuma_params_t* params_dev, int N, int E, int V, int M,
                  const float* W, const float* S, const float* B_init, const float* Wprev_init,
                  const yuma_outputs_t* out, void* workspace, size_t workspace_bytes,
                  int chunk_epochs, const yuma_run_options_t* opts, void* stream, float* phase_ms);
/* Slots of the bond history of an E-epoch run under these options:
 * hist_first < E ? (E - 1 - hist_first) / stride + 1 : 0 (stride 0 counts as
 * 1). Host only, needs no GPU. YUMA_EINVAL for E < 1 or a negative argument. */
int yuma_hist_slots(int E, int hist_stride, int hist_first);

/* 1 when yuma_run_ex / yuma_graph_create_ex with these arguments and
 * YUMA_RUN_W_U16 (`flags`: the run's other flags) read uint16 weights
 * natively, else 0. Host only, needs no GPU; of `out` it reads only which
 * pointers are non-NULL (NULL: nothing requested). Native: Yuma 3 and Yuma 4
 * (scalar or liquid alpha, any reset mode), V <= YUMA_REG_VALIDATORS,
 * M % 4 == 0, no YUMA_RUN_SHARED_INPUTS, none of Wn / Wc / Wb / B_inst / Tv
 * requested.                                                                */
int yuma_u16_native(int variant, int N, int E, int V, int M, const yuma_outputs_t* out,
                    int flags);

/* 1 when a run with these arguments and YUMA_RUN_HIST_BF16 (`flags`: the
 * run's other flags) writes its bond history as bfloat16, else 0. Host only,
 * needs no GPU; of `out` it reads only whether B_hist is non-NULL. Native:
 * Yuma 3 and Yuma 4 (scalar or liquid alpha, any reset mode), any V up to
 * YUMA_MAX_VALIDATORS, M % 4 == 0, no YUMA_RUN_SHARED_INPUTS, out->B_hist
 * requested. (A run also needs the alignment of the vector form: B_hist 8
 * bytes, W and the fp32 matrices as YUMA_RUN_W_U16 states.)                 */
int yuma_hist_bf16_native(int variant, int N, int E, int V, int M, const yuma_outputs_t* out,
                          int flags);

/* ------------------------------------------------------------------------
 * Input schedules: E epochs over K stored weight / stake slices.
 *
 * Simulated inputs are piecewise constant (every case of cases.py holds a
 * handful of matrices for tens of epochs; a convergence study holds one for
 * thousands). A request with a schedule (sched_dev != NULL or K != 0; the one
 * without the other is YUMA_EINVAL) takes the K distinct slices once, W [K][N][V][M]
 * (uint16 under YUMA_RUN_W_U16) and S [K][N][V], and a schedule sched_dev [E]
 * in DEVICE memory: epoch t reads slice sched_dev[t]. Every output has the
 * bits of yuma_run_opts on the expanded inputs W'[t] = W[sched[t]],
 * S'[t] = S[sched[t]]: the per-epoch outputs stay [E][N][..], B_hist keeps its
 * dense, strided or bfloat16 shape, reset_epoch stays an epoch index and the
 * conditional reset reads the previous epoch's consensus; the result does not
 * depend on chunk_epochs. Slices that no epoch references are allowed, and so
 * is K > E. The run stores K instead of E slices of W and makes the three
 * phase-1 passes over W (row sums, consensus, rank: pure functions of one
 * slice) once per stored slice instead of once per epoch; a gather kernel
 * copies their per-slice vectors into the per-epoch arrays, counted under
 * YUMA_PHASE_INCENTIVE in phase_ms.
 *
 * Native (yuma_sched_native returns 1): Yuma 3 and Yuma 4 (scalar or liquid
 * alpha, any reset mode), any V up to YUMA_MAX_VALIDATORS, M % 4 == 0 with
 * the alignments YUMA_RUN_W_U16 states (the vector form), no
 * YUMA_RUN_SHARED_INPUTS, none of Wn / Wc / Wb / B_inst / Tv / P / T
 * requested. Combines with YUMA_RUN_W_U16 (where yuma_u16_native holds), the
 * history stride and YUMA_RUN_HIST_BF16 (where yuma_hist_bf16_native holds)
 * as the dense run does; `flags` of yuma_sched_native are the run's flags.
 * Elsewhere the entry points return YUMA_EUNSUPPORTED before the first launch
 * and the caller expands the inputs itself.
 *
 * The host cannot check a schedule in device memory without a
 * synchronisation: every kernel that addresses memory through a schedule
 * entry clamps it into [0, K) first, so a bad schedule gives unspecified
 * numbers and never an access outside W and S. K < 1, a NULL sched_dev and
 * negative option fields return YUMA_EINVAL before the first launch. The
 * workspace is yuma_workspace_bytes_sched (>= yuma_workspace_bytes for the
 * same E, growing with K). A graph re-reads the schedule at every replay:
 * rewrite it in place between replays like any other input.
 * ---------------------------------------------------------------------- */
size_t yuma_workspace_bytes_sched(int variant, int N, int E, int K, int V, int M, int full_outputs);
/* The request of yuma_run_opts with K and sched_dev, both mandatory: K < 1, then
 * a NULL sched_dev are refused (YUMA_EINVAL) right after the options. */
int yuma_run_sched(int variant, const yuma_params_t* params_dev, int N, int E, int K, int V, int M,
                   const float* W, const float* S, const int32_t* sched_dev, const float* B_init,
                   const float* Wprev_init, const yuma_outputs_t* out, void* workspace,
                   size_t workspace_bytes, int chunk_epochs, const yuma_run_options_t* opts,
                   void* stream, float* phase_ms);
/* Host only, needs no GPU; of `out` it reads only which pointers are non-NULL. */
int yuma_sched_native(int variant, int N, int E, int K, int V, int M, const yuma_outputs_t* out,
                      int flags);

/* ------------------------------------------------------------------------
 * Watched bond columns: the bond history of a few miner columns.
 *
 * The charts that read a bond history plot a handful of servers (miner
 * columns); a [V][M] history per stored epoch is hundreds of times what they
 * read. YUMA_REQ_WATCH: a list watch_dev [n_watch] of miner columns in
 * DEVICE memory; the run writes B_watch [n_hist][N][V][n_watch] (fp32), n_hist =
 * yuma_hist_slots(E, stride, first) under the options' history stride and
 * first epoch, which apply to it as they do to B_hist: slot s, column j holds
 * the bits the dense history holds at [epoch t_s][n][v][watch_dev[j]].
 * Duplicated and unsorted columns are allowed. out->B_hist may be NULL -- the
 * intended use: the main run then takes its history-less scans, and a small
 * kernel of its own recomputes the watched elements from the per-epoch vectors
 * phase 1 leaves in the workspace (counted under YUMA_PHASE_BONDS) -- or
 * non-NULL: both histories are written. YUMA_RUN_HIST_BF16 concerns B_hist
 * only; B_watch is fp32. Every other output, B_final included, has the bits of
 * the same run without a watch list.
 *
 * sched_dev == NULL with K == 0 means no schedule: W is [E][N][V][M],
 * S [E][N][V] and the workspace yuma_workspace_bytes. With a schedule they are
 * the schedule's and the workspace is yuma_workspace_bytes_sched.
 * The watch list needs no workspace of its own.
 *
 * Native (yuma_watch_native returns 1; host only, `flags` are the run's
 * flags): Yuma 3 and Yuma 4 (scalar or liquid alpha, any reset mode), any V up
 * to YUMA_MAX_VALIDATORS, any M and any alignment (the kernel has scalar
 * accesses only), no YUMA_RUN_SHARED_INPUTS; with YUMA_RUN_W_U16 where
 * yuma_u16_native holds. Elsewhere the entry points return YUMA_EUNSUPPORTED
 * before the first launch and the caller gathers the columns of an fp32
 * history itself.
 *
 * The host cannot check a list in device memory without a synchronisation:
 * the kernel clamps every entry into [0, M) before it addresses anything, so a
 * bad list gives unspecified numbers and never an access outside W. A graph
 * re-reads the list at every replay: rewrite it in place between replays like
 * any other input.
 *
 * Refusals, in this order, all before the first launch and without a HIP call
 * (the graph form: the same code and yuma_last_error text, before the
 * capture opens): the options (as yuma_run_opts); [the graph handle]; sizes;
 * NULL params / W / S / out / workspace; a schedule pointer with K < 1, or
 * K != 0 without one (YUMA_EINVAL); n_watch < 1, then a NULL watch_dev or
 * B_watch (YUMA_EINVAL); the workspace size; the schedule not native; the
 * watch list not native (YUMA_EUNSUPPORTED); then YUMA_RUN_HIST_BF16 and
 * YUMA_RUN_W_U16 as ever. yuma_epoch and yuma_shard_stage take no watch list.
 * ---------------------------------------------------------------------- */
/* The request of yuma_run_sched's arguments (the schedule optional: NULL and
 * K = 0) with YUMA_REQ_WATCH always set: an empty list is refused. */
int yuma_run_watch(int variant, const yuma_params_t* params_dev, int N, int E, int K, int V, int M,
                   const float* W, const float* S, const int32_t* sched_dev, const float* B_init,
                   const float* Wprev_init, const yuma_outputs_t* out, const int32_t* watch_dev,
                   int n_watch, float* B_watch, void* workspace, size_t workspace_bytes,
                   int chunk_epochs, const yuma_run_options_t* opts, void* stream, float* phase_ms);
int yuma_watch_native(int variant, int N, int E, int V, int M, int n_watch, int flags);

/* ------------------------------------------------------------------------
 * Bond movement per epoch: when did the bonds stop moving.
 *
 * YUMA_REQ_MOVE: the run writes B_move [E][N][2] (fp32, device memory) beside
 * its other outputs:
 *   B_move[t][n][0] = max over (v, m) of |B_t[n][v][m] - B_{t-1}[n][v][m]|
 *   B_move[t][n][1] = max over (v, m) of |B_t[n][v][m]|
 * B_t is the bond state after epoch t, exactly the bits the dense fp32 history
 * holds; a reset at epoch t is therefore part of epoch t's movement. B_{-1} is
 * B_init, or all zeros when B_init is NULL. The difference is one fp32
 * subtraction and a maximum is order-independent, so the result is
 * bit-defined: it equals (hist[t] - hist[t-1]).abs().amax((-2, -1)) and
 * hist[t].abs().amax((-2, -1)) computed in fp32 on the dense history. NaN
 * propagates as in torch.amax: if any element's |difference| (or |B|) is NaN
 * the entry is a NaN with unspecified payload. -0 counts as +0. Every other
 * output, B_final included, keeps the bits of the same run without B_move, and
 * the result does not depend on chunk_epochs (across a chunk boundary the old
 * state is the one the scan loads from its state buffer).
 *
 * The history-less scan holds every element's old and new state in registers
 * at the update: it forms the two maxima there, reduces them over the wave and
 * parks them in LDS; every 256 epochs and at the end of a launch each wave sends
 * them as unsigned max atomics (one per maximum and epoch); the engine zeroes B_move
 * itself with a small kernel on the run's stream (inside a captured graph too:
 * every replay starts from zero). B_move needs no workspace of its own.
 *
 * Native (yuma_move_native returns 1; host only, makes no HIP call; of `out`
 * it reads only which pointers are non-NULL; `flags` are the run's flags):
 * Yuma 3 and Yuma 4 (scalar or liquid alpha, any reset mode), the vector form
 * (M % 4 == 0, with the alignments YUMA_RUN_W_U16 states), any V up to
 * YUMA_MAX_VALIDATORS, no YUMA_RUN_SHARED_INPUTS, out->B_hist NULL, none of
 * Wn / Wc / Wb / B_inst / Tv requested -- the calls whose scan is
 * YUMA_ELEM_FLAT1 / YUMA_ELEM_FLAT2. Within them it combines with
 * YUMA_RUN_W_U16 where yuma_u16_native holds (yuma_move_native tests it when
 * the flag is given), with a schedule where yuma_sched_native holds, and with
 * a watch list. Elsewhere the entry points return YUMA_EUNSUPPORTED before the
 * first launch and the caller reduces an fp32 history itself.
 *
 * Refusals, in this order, all before the first launch and without a HIP call
 * (the graph form: the same code and yuma_last_error text, before the
 * capture opens): the options (as yuma_run_opts); [the graph handle]; sizes;
 * NULL params / W / S / out / workspace; a schedule pointer with K < 1, or
 * K != 0 without one (YUMA_EINVAL); with a watch list (YUMA_REQ_WATCH),
 * n_watch < 1, then a NULL watch_dev or B_watch (YUMA_EINVAL);
 * a NULL B_move (YUMA_EINVAL); the workspace size; the schedule not native;
 * the watch list not native; the movement not native, then not in vector form
 * (YUMA_EUNSUPPORTED); then YUMA_RUN_HIST_BF16 and YUMA_RUN_W_U16 as ever.
 * yuma_epoch, yuma_shard_stage and the older entry points take no B_move.
 * ---------------------------------------------------------------------- */
/* yuma_run_watch's request with B_move and YUMA_REQ_MOVE always set (a NULL B_move is refused); YUMA_REQ_WATCH
 * is set when n_watch != 0 or either watch pointer is given: (NULL, 0, NULL) means "no watch list". */
int yuma_run_move(int variant, const yuma_params_t* params_dev, int N, int E, int K, int V, int M,
                  const float* W, const float* S, const int32_t* sched_dev, const float* B_init,
                  const float* Wprev_init, const yuma_outputs_t* out, const int32_t* watch_dev,
                  int n_watch, float* B_watch, float* B_move, void* workspace, size_t workspace_bytes,
                  int chunk_epochs, const yuma_run_options_t* opts, void* stream, float* phase_ms);
int yuma_move_native(int variant, int N, int E, int V, int M, const yuma_outputs_t* out, int flags);

/* ------------------------------------------------------------------------
 * Watched validator rows: the bond history of a few validators.
 *
 * The other half of the watch list's question: where are validator v's bonds
 * across all miners, and which miners pay it (D[v] = sum over m of B[v][m]
 * I[m])? YUMA_REQ_ROWS: a list rows_dev [n_rows] of validator indices in
 * DEVICE memory; the run writes B_rows [n_hist][N][n_rows][M] (fp32), n_hist =
 * yuma_hist_slots(E, stride, first) under the options' history stride and
 * first epoch: slot s, row j holds the bits the dense history holds at
 * [epoch t_s][n][rows_dev[j]][0 .. M). Duplicated and unsorted rows are
 * allowed. out->B_hist may be NULL -- the intended use: the main run takes its
 * history-less scans, and a small kernel of its own (k_bonds_rows, counted
 * under YUMA_PHASE_BONDS) recomputes the watched rows from the per-epoch
 * vectors phase 1 leaves in the workspace -- or non-NULL: both histories are
 * written. YUMA_RUN_HIST_BF16 concerns B_hist only; B_rows is fp32. Every
 * other output, B_final included, has the bits of the same run without a row
 * list. The row list needs no workspace of its own.
 *
 * Native (yuma_rows_native returns 1; host only, makes no HIP call; `flags`
 * are the run's flags): Yuma 3 and Yuma 4 (scalar or liquid alpha, any reset
 * of the parameter record), any V up to YUMA_MAX_VALIDATORS, any M and any
 * alignment (four columns per thread in 16-byte accesses where M % 4 == 0 and
 * W, B_init, the state, bond_alpha and B_rows are aligned for them; one
 * column per thread elsewhere), no YUMA_RUN_SHARED_INPUTS; with
 * YUMA_RUN_W_U16 where yuma_u16_native holds. Elsewhere the entry points
 * return YUMA_EUNSUPPORTED before the first launch and the caller gathers the
 * rows of an fp32 history itself.
 *
 * The host cannot check a list in device memory without a synchronisation:
 * the kernel clamps every entry into [0, V) before it addresses anything, so a
 * bad entry gives unspecified numbers and never an access outside a buffer. A
 * graph re-reads the list at every replay: rewrite it in place between
 * replays like any other input.
 *
 * Refusals, in this order, all before the first launch and without a HIP call
 * (the graph form: the same code and yuma_last_error text, before the
 * capture opens): the options (as yuma_run_opts); [the graph handle]; sizes;
 * NULL params / W / S / out / workspace; a schedule pointer with K < 1, or
 * K != 0 without one (YUMA_EINVAL); with a watch list (YUMA_REQ_WATCH),
 * n_watch < 1, then a NULL watch_dev or B_watch (YUMA_EINVAL);
 * n_rows < 1, then a NULL rows_dev or B_rows, then a grid of N n_rows
 * ceil(M / 64) blocks beyond INT_MAX (YUMA_EINVAL); the workspace size; the
 * schedule not native; the watch list not native; with YUMA_REQ_MOVE, the
 * movement not native, then not in vector form; the row list not native
 * (YUMA_EUNSUPPORTED); then YUMA_RUN_HIST_BF16 and YUMA_RUN_W_U16 as ever.
 * yuma_epoch, yuma_shard_stage and the older entry points take no row list.
 * ---------------------------------------------------------------------- */
/* yuma_run_move's request with the row list and YUMA_REQ_ROWS always set (an empty list is refused); YUMA_REQ_MOVE
 * is set when B_move != NULL (NULL means "no movement output"), YUMA_REQ_WATCH as in yuma_run_move. */
int yuma_run_rows(int variant, const yuma_params_t* params_dev, int N, int E, int K, int V, int M,
                  const float* W, const float* S, const int32_t* sched_dev, const float* B_init,
                  const float* Wprev_init, const yuma_outputs_t* out, const int32_t* watch_dev,
                  int n_watch, float* B_watch, float* B_move, const int32_t* rows_dev, int n_rows,
                  float* B_rows, void* workspace, size_t workspace_bytes, int chunk_epochs,
                  const yuma_run_options_t* opts, void* stream, float* phase_ms);
int yuma_rows_native(int variant, int N, int E, int V, int M, int n_rows, int flags);

/* ------------------------------------------------------------------------
 * Per-validator bond summary per epoch: which validator's bonds still move,
 * how large is each validator's position, when did each one settle.
 *
 * YUMA_REQ_ROWSTAT: the run writes B_rowstat [E][N][V][3] (fp32, device memory)
 * beside its other outputs. B_t is the bond state after epoch t, exactly the
 * bits the dense fp32 history holds; B_{-1} is B_init, or zeros without one.
 *   B_rowstat[t][n][v][0] = max over m of |B_t[n][v][m] - B_{t-1}[n][v][m]|
 *   B_rowstat[t][n][v][1] = max over m of |B_t[n][v][m]|
 *   B_rowstat[t][n][v][2] = sum over m of B_t[n][v][m]
 * [0] and [1] are yuma_run_move's two maxima taken over one row: one fp32
 * subtraction per element, a reset at t counts as movement, NaN as in
 * torch.amax, -0 counts as +0; bit-equal to (hist[t] - hist[t-1]).abs()
 * .amax(-1) and hist[t].abs().amax(-1) on the dense history, and their
 * maximum over v is B_move[t][n] bit for bit.
 * [2] is summed in the canonical order of the dividend partials with every
 * incentive replaced by 1. Per 64-miner tile: each lane adds its four
 * consecutive columns in order starting from +0, and the tile's 16 lanes are
 * joined by the xor-butterfly tree (lane distances 1, 2, 4, 8). Tiles p_k are
 * joined into quads Q_b = (p_4b + p_4b+1) + (p_4b+2 + p_4b+3), absent tiles
 * counting 0; S_g is the sequential sum of the quads b = g (mod 4), and the
 * total is ((S_0 + S_1) + S_2) + S_3 -- the order that gives D. The bits are
 * the same on both native scan shapes and for every chunk_epochs.
 * Every other output, B_final included, keeps the bits of the same run
 * without B_rowstat.
 *
 * The history-less scan forms all three at the update: the maxima go out as
 * unsigned max atomics, one per row, statistic, epoch and 256-miner column
 * block, into B_rowstat, which the engine zeroes itself with a small kernel
 * on the run's stream (inside a captured graph too: every replay starts from
 * zero); the totals go through a second array of quad partials in the
 * workspace (yuma_workspace_bytes_rowstat >= yuma_workspace_bytes) and a twin
 * of the dividends' summing kernel.
 *
 * Watch and row lists are kernels of their own and combine with the summary. A
 * schedule pointer or YUMA_REQ_MOVE does not: YUMA_EUNSUPPORTED.
 *
 * Native (yuma_rowstat_native returns 1; host only, makes no HIP call; of
 * `out` it reads only which pointers are non-NULL; `flags` are the run's
 * flags): Yuma 3 and Yuma 4 (scalar or liquid alpha, any reset of the
 * parameter record), the vector form (M % 4 == 0; W and the fp32 matrices
 * 16-byte aligned), any V up to YUMA_MAX_VALIDATORS, no
 * YUMA_RUN_SHARED_INPUTS, YUMA_RUN_W_U16 or YUMA_RUN_HIST_BF16, out->B_hist
 * NULL, none of Wn / Wc / Wb / B_inst / Tv requested -- the calls whose scan
 * is YUMA_ELEM_FLAT1 / YUMA_ELEM_FLAT2 on fp32 weights. Elsewhere the entry
 * points return YUMA_EUNSUPPORTED before the first launch and the caller
 * reduces an fp32 history itself. yuma_scan_plan_t has no room for a further
 * field at its fixed size, so yuma_scan_plan reports the shape of such a run
 * (FLAT1 / FLAT2) and not the summary form.
 *
 * Refusals, in this order, all before the first launch and without a HIP call
 * (the graph form: the same code and yuma_last_error text, before
 * the capture opens): as the row list's section up to the row list's own (which
 * apply only with YUMA_REQ_ROWS); a NULL B_rowstat (YUMA_EINVAL); the workspace
 * size (yuma_workspace_bytes_rowstat); the schedule, watch list, movement and
 * row list refusals of yuma_run_rows; a schedule pointer, a B_move or reset
 * events beside the summary; the summary not native; then not in vector form
 * (YUMA_EUNSUPPORTED); then YUMA_RUN_HIST_BF16 and YUMA_RUN_W_U16 as ever.
 * ---------------------------------------------------------------------- */
size_t yuma_workspace_bytes_rowstat(int variant, int N, int E, int V, int M, int full_outputs);
/* yuma_run_rows's request with B_rowstat and YUMA_REQ_ROWSTAT always set (a NULL B_rowstat is refused); here
 * YUMA_REQ_ROWS too is set only when n_rows != 0 or either row pointer is given. */
int yuma_run_rowstat(int variant, const yuma_params_t* params_dev, int N, int E, int K, int V, int M,
                     const float* W, const float* S, const int32_t* sched_dev, const float* B_init,
                     const float* Wprev_init, const yuma_outputs_t* out, const int32_t* watch_dev,
                     int n_watch, float* B_watch, float* B_move, const int32_t* rows_dev, int n_rows,
                     float* B_rows, float* B_rowstat, void* workspace, size_t workspace_bytes,
                     int chunk_epochs, const yuma_run_options_t* opts, void* stream, float* phase_ms);
int yuma_rowstat_native(int variant, int N, int E, int V, int M, const yuma_outputs_t* out, int flags);

/* ------------------------------------------------------------------------
 * Bond reset events: any number of column resets inside one run.
 *
 * A subnet deregisters miners all the time, and every deregistration clears
 * that UID's bonds; yuma_params_t carries one reset per scenario and run.
 * YUMA_REQ_RESETS: a list events_dev [n_events] of yuma_reset_event_t in
 * DEVICE memory. An event (epoch t, scenario n, column c, mode) applies
 * B[n][:, c] = 0 before epoch t's update of scenario n, if a bond state exists
 * and the mode's rule holds:
 *  - a bond state exists when t >= 1, or t == 0 and B_init is given;
 *  - YUMA_RESET_ALWAYS always fires;
 *  - YUMA_RESET_IF_ZERO_CONSENSUS fires iff t >= 1 and C[t-1][n][c] == 0.0f,
 *    C the quantised server_consensus_weight (at t == 0 it never fires, as
 *    the scenario's own conditional reset);
 *  - c == -1 means every column, for YUMA_RESET_ALWAYS only; with the
 *    conditional mode such an event is ignored;
 *  - duplicates are allowed and the order does not matter;
 *  - an event whose epoch is outside [0, E), scenario outside [0, N), column
 *    outside [-1, M) or mode any other value is ignored by the device code
 *    and never causes an access outside a buffer (the host cannot check a list
 *    in device memory without a synchronisation);
 *  - the scenario's own reset in yuma_params_t keeps working beside the events.
 * The history holds the state after the update, so a reset at t shows in slot
 * t. Every output has the bits of the chain of yuma_run_opts calls cut at the
 * event epochs, each resumed from the previous B_final with the columns
 * zeroed; the result does not depend on chunk_epochs (an event at a chunk's
 * first epoch reads C of the previous chunk's last epoch).
 *
 * Without the section the run is exactly yuma_run_opts: the same launches
 * and the yuma_workspace_bytes size. With it the workspace is
 * yuma_workspace_bytes_resets (>= yuma_workspace_bytes): the difference is a
 * table of one bit per (epoch, scenario, column), bytes [E][N][ceil(M / 8)],
 * which the engine zeroes with a small kernel and a resolve kernel (one thread
 * per event, after the phase that leaves C) fills with atomic ORs; the bond
 * scan loads a lane's nibble of it beside its other per-epoch inputs and
 * clears the state with an AND mask, branch-free. A graph re-reads the list at every replay:
 * rewrite it in place between replays like any other input.
 *
 * Native (yuma_resets_native returns 1; host only, makes no HIP call; of `out`
 * it reads only which pointers are non-NULL; `flags` are the run's flags):
 * Yuma 3 and Yuma 4 (scalar or liquid alpha, any params reset), the vector
 * form (M % 4 == 0, with the alignments YUMA_RUN_W_U16 states), fp32 weights,
 * any V up to YUMA_MAX_VALIDATORS, no YUMA_RUN_SHARED_INPUTS, no
 * YUMA_RUN_W_U16, no YUMA_RUN_HIST_BF16, none of Wn / Wc / Wb / B_inst / Tv
 * requested; the fp32 history dense, strided or absent -- the calls whose scan
 * is YUMA_ELEM_WIDE, YUMA_ELEM_TILE_HIST, YUMA_ELEM_FLAT1 or YUMA_ELEM_FLAT2.
 * Elsewhere the entry points return YUMA_EUNSUPPORTED before the first launch
 * and the caller cuts the run at the event epochs itself. Events (of either
 * kind) beside a schedule, a watch list, B_move, a row list or the row summary
 * have never run: a request that asks for both is YUMA_EUNSUPPORTED.
 *
 * Refusals, in this order, all before the first launch and without a HIP call
 * (the graph form: the same code and yuma_last_error text, before
 * the capture opens): the options (as yuma_run_opts); [the graph handle];
 * sizes; NULL params / W / S / out / workspace; n_events < 0, then
 * n_events > 0 with a NULL list (YUMA_EINVAL); the workspace size
 * (YUMA_EWORKSPACE); a section the events do not combine with; the events not
 * native, then not in vector form (YUMA_EUNSUPPORTED).
 * ---------------------------------------------------------------------- */
typedef struct yuma_reset_event {
  int32_t epoch;    /* the reset precedes this epoch's update                  */
  int32_t scenario; /* 0 <= scenario < N                                       */
  int32_t column;   /* miner column, or -1: every column (YUMA_RESET_ALWAYS)   */
  int32_t mode;     /* YUMA_RESET_ALWAYS or YUMA_RESET_IF_ZERO_CONSENSUS       */
} yuma_reset_event_t; /* 16 bytes */
size_t yuma_workspace_bytes_resets(int variant, int N, int E, int V, int M, int full_outputs);
/* yuma_run_opts's request with the event list; YUMA_REQ_RESETS is set when n_events != 0 or events_dev != NULL:
 * (NULL, 0) means "no events". */
int yuma_run_resets(int variant, const yuma_params_t* params_dev, int N, int E, int V, int M,
                    const float* W, const float* S, const float* B_init, const float* Wprev_init,
                    const yuma_outputs_t* out, const yuma_reset_event_t* events_dev, int n_events,
                    void* workspace, size_t workspace_bytes, int chunk_epochs,
                    const yuma_run_options_t* opts, void* stream, float* phase_ms);
int yuma_resets_native(int variant, int N, int E, int V, int M, const yuma_outputs_t* out, int flags);

/* ------------------------------------------------------------------------
 * Validator-row events: bond rows zeroed at any epoch inside one run.
 *
 * A validator that leaves or whose hotkey is replaced has its bond row
 * cleared. YUMA_REQ_ROW_EVENTS: a second list, row_events_dev [n_row_events]
 * of yuma_row_event_t in DEVICE memory, with or without YUMA_REQ_RESETS. A row event (epoch t, scenario n, row v) applies B[n][v][:] = 0
 * before epoch t's update of scenario n, if a bond state exists (t >= 1, or
 * t == 0 and B_init is given):
 *  - the event is unconditional: no consensus rule applies to a validator;
 *  - duplicates are allowed and the order does not matter; row events commute
 *    with the column events of the same epoch (both store +0);
 *  - an event whose epoch is outside [0, E), scenario outside [0, N), row
 *    outside [0, V) or reserved word non-zero is ignored by the device code
 *    and never causes an access outside a buffer;
 *  - the column events and the scenario's own reset in yuma_params_t keep
 *    working beside the row events.
 * The history holds the state after the update, so a row reset at t shows in
 * slot t, and Dn[t][n][v] is the dividend of the fresh row. Every output has
 * the bits of the chain of yuma_run_opts calls cut at the event epochs, each
 * resumed from the previous B_final with the rows and columns zeroed; the
 * result does not depend on chunk_epochs.
 *
 * Without the section the run is exactly that of YUMA_REQ_RESETS alone: the same
 * launches and the same workspace requirement (without either section,
 * yuma_run_opts's). With it the workspace is
 * yuma_workspace_bytes_events (>= yuma_workspace_bytes_resets): the difference
 * is the row table, one 32-BIT WORD per (epoch, scenario, validator), words
 * [E][N][V] -- the index of the scan's other per-row inputs -- padded to 256
 * bytes, behind the column table. Zero keeps the row; the resolve kernel (one
 * thread per event, every field range-checked before anything is addressed)
 * sets every bit of the word with an integer atomic OR. The engine zeroes both
 * tables with a small kernel, so inside a captured graph every replay starts
 * from zero and re-reads both lists. The bond scan with both tables loads the
 * R words of a lane's R rows beside the column byte, first in its fetch, and
 * clears row i with an AND mask, branch-free; a run without column events
 * runs it on an all-zero column table.
 *
 * Native (yuma_events_native, host only, no HIP call): exactly the set of
 * yuma_resets_native. Refusals are yuma_run_resets's, in its order, with two
 * inserted after the column list's checks: n_row_events < 0, then
 * n_row_events > 0 with a NULL list (YUMA_EINVAL); and one appended at the end:
 * N * V >= 2^29 with a row list (YUMA_EUNSUPPORTED: the scan steps through the
 * row table by one epoch's N * V words as a 32-bit count of bytes; such a run's
 * row table alone exceeds 2 GiB per epoch). All come before the first
 * launch and without a HIP call (the graph form: the same code and
 * yuma_last_error text, before the capture opens).
 * ---------------------------------------------------------------------- */
typedef struct yuma_row_event {
  int32_t epoch;    /* the reset precedes this epoch's update */
  int32_t scenario; /* 0 <= scenario < N                      */
  int32_t row;      /* validator row, 0 <= row < V            */
  int32_t reserved; /* must be 0                              */
} yuma_row_event_t; /* 16 bytes */
size_t yuma_workspace_bytes_events(int variant, int N, int E, int V, int M, int full_outputs);
/* yuma_run_resets's request with the row event list after n_events; YUMA_REQ_ROW_EVENTS is set when
 * n_row_events != 0 or row_events_dev != NULL. */
int yuma_run_events(int variant, const yuma_params_t* params_dev, int N, int E, int V, int M,
                    const float* W, const float* S, const float* B_init, const float* Wprev_init,
                    const yuma_outputs_t* out, const yuma_reset_event_t* events_dev, int n_events,
                    const yuma_row_event_t* row_events_dev, int n_row_events,
                    void* workspace, size_t workspace_bytes, int chunk_epochs,
                    const yuma_run_options_t* opts, void* stream, float* phase_ms);
int yuma_events_native(int variant, int N, int E, int V, int M, const yuma_outputs_t* out, int flags);

/* ------------------------------------------------------------------------
 * The run request: one record behind every run and graph entry point.
 *
 * A run is the base fields (what yuma_run_opts takes, and a schedule) plus any
 * of six sections, each described in its block above. A section is present by
 * its bit in `sections` and by nothing else: with the bit set its fields are
 * checked as that block states (a NULL or empty list is then YUMA_EINVAL);
 * with the bit clear they must be NULL / 0 (YUMA_EINVAL otherwise). The
 * positional entry points differ only in which NULLs they read as "absent":
 * each states its mask beside its prototype. A schedule has no bit: it is
 * present when sched_dev != NULL or K != 0.
 *
 * Refusals, all before the first launch and without a HIP call, alike from
 * yuma_run_request and yuma_graph_create_request (the same code and
 * yuma_last_error text, before the capture opens): a NULL request; struct_size
 * != sizeof(yuma_request_t); an unknown section bit; a non-zero reserved word;
 * the options (as yuma_run_opts); a field of an absent section given (all
 * YUMA_EINVAL); [the graph handle]; then sizes, NULL params / W / S / out /
 * workspace, the schedule, and each present section's refusals in the order
 * its block gives, the workspace size between the YUMA_EINVAL and the
 * YUMA_EUNSUPPORTED ones. The workspace is yuma_workspace_bytes_request.
 * A later library version appends fields in place of reserved words and keeps
 * the size; a library refuses a record of any other size.
 * ---------------------------------------------------------------------- */
enum yuma_request_sections {
  YUMA_REQ_WATCH = 1,      /* watch_dev, n_watch, B_watch          */
  YUMA_REQ_MOVE = 2,       /* B_move                               */
  YUMA_REQ_ROWS = 4,       /* rows_dev, n_rows, B_rows             */
  YUMA_REQ_ROWSTAT = 8,    /* B_rowstat                            */
  YUMA_REQ_RESETS = 16,    /* events_dev, n_events                 */
  YUMA_REQ_ROW_EVENTS = 32 /* row_events_dev, n_row_events         */
};
typedef struct yuma_request {
  uint32_t struct_size;    /* sizeof(yuma_request_t)                                */
  uint32_t sections;       /* yuma_request_sections                                 */
  int32_t variant;         /* yuma_variant                                          */
  int32_t N, E;            /* scenarios, epochs                                     */
  int32_t K;               /* stored slices under a schedule, else 0                */
  int32_t V, M;            /* validators, miners                                    */
  const yuma_params_t* params_dev; /* [N], device memory                            */
  const void* W;           /* [E or K][N][V][M] fp32 (uint16: YUMA_RUN_W_U16)       */
  const float* S;          /* [E or K][N][V]                                        */
  const int32_t* sched_dev;/* [E] slice per epoch, or NULL: no schedule             */
  const float* B_init;     /* [N][V][M] or NULL                                     */
  const float* Wprev_init; /* Yuma2: [N][V][M] or NULL                              */
  const yuma_outputs_t* out;
  void* workspace;
  size_t workspace_bytes;
  const yuma_run_options_t* opts; /* NULL: every default                            */
  const int32_t* watch_dev;/* YUMA_REQ_WATCH: [n_watch] miner columns               */
  float* B_watch;          /*   [n_hist][N][V][n_watch]                             */
  float* B_move;           /* YUMA_REQ_MOVE: [E][N][2]                              */
  const int32_t* rows_dev; /* YUMA_REQ_ROWS: [n_rows] validator rows                */
  float* B_rows;           /*   [n_hist][N][n_rows][M]                              */
  float* B_rowstat;        /* YUMA_REQ_ROWSTAT: [E][N][V][3]                        */
  const yuma_reset_event_t* events_dev;   /* YUMA_REQ_RESETS: [n_events]            */
  const yuma_row_event_t* row_events_dev; /* YUMA_REQ_ROW_EVENTS: [n_row_events]    */
  int32_t chunk_epochs;    /* epochs per phase-1 batch (0 = engine default)         */
  int32_t n_watch, n_rows, n_events, n_row_events;
  int32_t reserved[15];    /* must be 0                                             */
} yuma_request_t;          /* 256 bytes */
/* stream: a hipStream_t, NULL = default stream. phase_ms: NULL, or per-phase
 * device time as yuma_run_profiled (blocks). */
int yuma_run_request(const yuma_request_t* request, void* stream, float* phase_ms);
/* Bytes of workspace the request needs. Reads the sizes, K, `sections` and
 * whether out->Tv is requested (out may be NULL: not requested); equals the
 * yuma_workspace_bytes* function of the same shape. 0 for a NULL request, a
 * wrong struct_size, a non-positive size or K < 0. */
size_t yuma_workspace_bytes_request(const yuma_request_t* request);

/* ------------------------------------------------------------------------
 * Which bond scan a call reaches. Host only, needs no GPU and makes no HIP
 * call: the engine's own choice (the function its runs call before they launch
 * the scan), reported for the first chunk of yuma_run_opts / yuma_run_sched
 * (has_sched != 0) with these arguments, or for stage 4 of yuma_shard_stage
 * (shard_stage != 0: no options, no schedule). Of `out` it reads only which
 * pointers are non-NULL. vector_form is given, not derived from buffers: 1
 * for M % 4 == 0 and aligned matrices (see YUMA_RUN_W_U16), 0 for the scalar
 * form. Returns YUMA_OK and fills *plan, or the code the run returns for
 * sizes, options, or a schedule / YUMA_RUN_W_U16 / YUMA_RUN_HIST_BF16 that is
 * not native or not in vector form. The kernels and their flags are described
 * in DESIGN.md section 2.0.
 * ---------------------------------------------------------------------- */
enum { /* yuma_scan_plan_t.form: the kernel */
  YUMA_SCAN_TILE = 0,     /* k_bonds: a block owns the columns of a 64-miner tile    */
  YUMA_SCAN_STRIP = 1,    /* k_bonds_cn: a block owns a 16-miner strip               */
  YUMA_SCAN_RUST_BIG = 2, /* k_rust_big_ema + k_rust_big_norm, one pair per epoch    */
  YUMA_SCAN_ELEM = 3,     /* k_bonds_elem                                            */
  YUMA_SCAN_GRP = 4       /* k_bonds_grp: the shared-input sweep scan                */
};
enum { /* yuma_scan_plan_t.shape: k_bonds_elem's block shape */
  YUMA_ELEM_NONE = 0,      /* (another kernel)                                       */
  YUMA_ELEM_WIDE = 1,      /* 512 threads x 1024 miners, 2 rows, the history         */
  YUMA_ELEM_TILE_HIST = 2, /* 256 threads on 64-miner tiles, 2 rows, the history     */
  YUMA_ELEM_TILE = 3,      /* ... without the history                                */
  YUMA_ELEM_FLAT1 = 4,     /* 256 threads x 256 miners, 1 row                        */
  YUMA_ELEM_FLAT2 = 5      /* ... 2 rows                                             */
};
enum { YUMA_SCAN_HIST_NONE = 0, YUMA_SCAN_HIST_FP32 = 1, YUMA_SCAN_HIST_BF16 = 2 };
enum { /* yuma_scan_plan_t.dpl: layout of the dividend partials */
  YUMA_DP_TV = 0, /* [slice][tile][V]             */
  YUMA_DP_VQ = 1, /* [slice][V][quad]             */
  YUMA_DP_QTE = 2 /* [scenario][quad][V][epoch]   */
};
typedef struct {
  long long grid;      /* blocks of the launch                                     */
  int32_t variant;     /* as given                                                 */
  int32_t vector_form; /* as given                                                 */
  int32_t w_u16;       /* W element type: uint16 (YUMA_RUN_W_U16)                  */
  int32_t form;        /* YUMA_SCAN_*                                              */
  int32_t shape;       /* YUMA_ELEM_*                                              */
  int32_t rows;        /* rows per lane (k_bonds: rows per thread)                 */
  int32_t rq;          /* RQ: divides by k_rowsum's screened reciprocals           */
  int32_t hs;          /* HS: a strided history                                    */
  int32_t hist;        /* a history is written                                     */
  int32_t nt;          /* NT: non-temporal history stores (k_bonds_elem)           */
  int32_t hist_bf16;   /* HT: the history's elements are bfloat16                  */
  int32_t sc;          /* SC: under an input schedule                              */
  int32_t rowblocks;   /* row blocks per scenario and column block                 */
  int32_t cblocks;     /* column blocks                                            */
  int32_t block;       /* threads per block                                        */
  int32_t ptiles;      /* dividend partials per slice and validator                */
  int32_t dpl;         /* YUMA_DP_*                                                */
  int32_t rc;          /* k_bonds: 0 256 threads x 1 row, 1 256 x 4, 2 256 x 16, 3 1024 x 16 */
} yuma_scan_plan_t;    /* 80 bytes */
int yuma_scan_plan(int variant, int N, int E, int V, int M, const yuma_outputs_t* out,
                   const yuma_run_options_t* opts, int vector_form, int has_sched, int shard_stage,
                   yuma_scan_plan_t* plan);

/* hipGraph form of yuma_run: the whole multi-epoch run (every phase of every
 * chunk, no host work between them) captured once into a HIP graph and
 * replayed with one hipGraphLaunch. The arguments are those of yuma_run and
 * are baked into the graph: every replay reads the same W / S / params /
 * B_init buffers (refill them in place between replays) and writes the same
 * outputs. Capture happens on an internal stream; `stream` orders the capture
 * after the caller's prior work only through the caller's own sync, so call
 * it with inputs already resident. Replaces the per-epoch Python loop of
 * run_simulation (simulation_utils.py:52-110) for repeated runs.
 * Every yuma_graph_create* reads its flags / options / schedule as its run
 * entry point does, then checks `graph` (NULL: YUMA_EINVAL; else *graph = NULL
 * until the graph exists), then validates the rest exactly as that run entry
 * point does, in its order, before the capture opens: the same code and
 * yuma_last_error text, and nothing is refused inside an open capture.      */
typedef struct yuma_graph* yuma_graph_t;
int yuma_graph_create(yuma_graph_t* graph, int variant, const yuma_params_t* params_dev, int N,
                      int E, int V, int M, const float* W, const float* S,
                      const float* B_init, const float* Wprev_init, const yuma_outputs_t* out,
                      void* workspace, size_t workspace_bytes, int chunk_epochs);
/* yuma_graph_create with yuma_run_ex's flags. */
int yuma_graph_create_ex(yuma_graph_t* graph, int variant, const yuma_params_t* params_dev, int N,
                         int E, int V, int M, const float* W, const float* S,
                         const float* B_init, const float* Wprev_init, const yuma_outputs_t* out,
                         void* workspace, size_t workspace_bytes, int chunk_epochs, int flags);
/* yuma_graph_create with yuma_run_opts's options (the history stride). */
int yuma_graph_create_opts(yuma_graph_t* graph, int variant, const yuma_params_t* params_dev, int N,
                           int E, int V, int M, const float* W, const float* S,
                           const float* B_init, const float* Wprev_init, const yuma_outputs_t* out,
                           void* workspace, size_t workspace_bytes, int chunk_epochs,
                           const yuma_run_options_t* opts);
/* yuma_graph_create_opts under an input schedule (yuma_run_sched's arguments). */
int yuma_graph_create_sched(yuma_graph_t* graph, int variant, const yuma_params_t* params_dev, int N,
                            int E, int K, int V, int M, const float* W, const float* S,
                            const int32_t* sched_dev, const float* B_init, const float* Wprev_init,
                            const yuma_outputs_t* out, void* workspace, size_t workspace_bytes,
                            int chunk_epochs, const yuma_run_options_t* opts);
/* yuma_graph_create_sched with a watch list (yuma_run_watch's arguments). */
int yuma_graph_create_watch(yuma_graph_t* graph, int variant, const yuma_params_t* params_dev, int N,
                            int E, int K, int V, int M, const float* W, const float* S,
                            const int32_t* sched_dev, const float* B_init, const float* Wprev_init,
                            const yuma_outputs_t* out, const int32_t* watch_dev, int n_watch,
                            float* B_watch, void* workspace, size_t workspace_bytes,
                            int chunk_epochs, const yuma_run_options_t* opts);
/* yuma_graph_create_watch with the bond movement (yuma_run_move's arguments). */
int yuma_graph_create_move(yuma_graph_t* graph, int variant, const yuma_params_t* params_dev, int N,
                           int E, int K, int V, int M, const float* W, const float* S,
                           const int32_t* sched_dev, const float* B_init, const float* Wprev_init,
                           const yuma_outputs_t* out, const int32_t* watch_dev, int n_watch,
                           float* B_watch, float* B_move, void* workspace, size_t workspace_bytes,
                           int chunk_epochs, const yuma_run_options_t* opts);
/* yuma_graph_create_move with a row list (yuma_run_rows's arguments). */
int yuma_graph_create_rows(yuma_graph_t* graph, int variant, const yuma_params_t* params_dev, int N,
                           int E, int K, int V, int M, const float* W, const float* S,
                           const int32_t* sched_dev, const float* B_init, const float* Wprev_init,
                           const yuma_outputs_t* out, const int32_t* watch_dev, int n_watch,
                           float* B_watch, float* B_move, const int32_t* rows_dev, int n_rows,
                           float* B_rows, void* workspace, size_t workspace_bytes, int chunk_epochs,
                           const yuma_run_options_t* opts);
/* yuma_graph_create_rows with the row summary (yuma_run_rowstat's arguments). */
int yuma_graph_create_rowstat(yuma_graph_t* graph, int variant, const yuma_params_t* params_dev, int N,
                              int E, int K, int V, int M, const float* W, const float* S,
                              const int32_t* sched_dev, const float* B_init, const float* Wprev_init,
                              const yuma_outputs_t* out, const int32_t* watch_dev, int n_watch,
                              float* B_watch, float* B_move, const int32_t* rows_dev, int n_rows,
                              float* B_rows, float* B_rowstat, void* workspace, size_t workspace_bytes,
                              int chunk_epochs, const yuma_run_options_t* opts);
/* yuma_graph_create_opts with reset events (yuma_run_resets's arguments). */
int yuma_graph_create_resets(yuma_graph_t* graph, int variant, const yuma_params_t* params_dev, int N,
                             int E, int V, int M, const float* W, const float* S,
                             const float* B_init, const float* Wprev_init, const yuma_outputs_t* out,
                             const yuma_reset_event_t* events_dev, int n_events, void* workspace,
                             size_t workspace_bytes, int chunk_epochs, const yuma_run_options_t* opts);
/* yuma_graph_create_resets with validator-row events (yuma_run_events's arguments). */
int yuma_graph_create_events(yuma_graph_t* graph, int variant, const yuma_params_t* params_dev, int N,
                             int E, int V, int M, const float* W, const float* S,
                             const float* B_init, const float* Wprev_init, const yuma_outputs_t* out,
                             const yuma_reset_event_t* events_dev, int n_events,
                             const yuma_row_event_t* row_events_dev, int n_row_events, void* workspace,
                             size_t workspace_bytes, int chunk_epochs, const yuma_run_options_t* opts);
/* The graph of a request: what every yuma_graph_create* above calls with its run twin's record. */
int yuma_graph_create_request(yuma_graph_t* graph, const yuma_request_t* request);
/* Replay on `stream` (stream-ordered, no host synchronisation). */
int yuma_graph_launch(yuma_graph_t graph, void* stream);
/* Kernel nodes in the captured graph (diagnostics / tests). */
int yuma_graph_nodes(yuma_graph_t graph);
int yuma_graph_destroy(yuma_graph_t graph);

/* Phases of a run, in launch order (per chunk of epochs). */
enum yuma_phase {
  YUMA_PHASE_ROWSUM = 0,    /* k_rowsum:    row sums, stake normalisation      */
  YUMA_PHASE_CONSENSUS = 1, /* k_consensus: bisection per miner column          */
  YUMA_PHASE_QUANTISE = 2,  /* k_quantise:  C quantisation, liquid alpha        */
  YUMA_PHASE_RANK = 3,      /* k_rank:      clip, rank                          */
  YUMA_PHASE_INCENTIVE = 4, /* k_incentive: incentive, trust                    */
  YUMA_PHASE_BONDS = 5,     /* k_bonds:     bond recurrence over the chunk      */
  YUMA_PHASE_FINALIZE = 6,  /* k_finalize:  dividends                           */
  YUMA_NUM_PHASES = 7
};

/* yuma_run plus per-phase device time: HIP events are recorded on `stream`
 * between phases and phase_ms[YUMA_NUM_PHASES] receives the milliseconds
 * spent in each phase summed over chunks. Blocks until
 * the stream reaches the end of the run. For benchmarks / roofline only. */
int yuma_run_profiled(int variant, const yuma_params_t* params_dev, int N, int E, int V, int M,
                      const float* W, const float* S, const float* B_init,
                      const float* Wprev_init, const yuma_outputs_t* out, void* workspace,
                      size_t workspace_bytes, int chunk_epochs, void* stream, float* phase_ms);

/* One call of a Yuma* variant for N independent slices (E = 1):
 * yumas.py:61 (YumaRust), :175 (Yuma), :285 (Yuma2, W_prev may be NULL),
 * :399 (Yuma3), :494 (Yuma4). B_old may be NULL (first epoch).             */
int yuma_epoch(int variant, const yuma_params_t* params_dev, int N, int V, int M,
               const float* W, const float* W_prev, const float* S, const float* B_old,
               const yuma_outputs_t* out, void* workspace, size_t workspace_bytes,
               void* stream);

/* ------------------------------------------------------------------------
 * Miner-column sharding of one wide subnet.
 *
 * The reference runs a wide subnet as one Yuma* call per epoch
 * (yumas.py:399 etc., driven by run_simulation, simulation_utils.py:44-110).
 * Every cross-miner quantity of that epoch step is a sum over miner columns
 * (row sums :186, sum C :211, sum R :220, D :261/:474/:589) or a quantile of
 * C (:231-247), and the bond recurrence is column-local, so a process can own
 * columns [col0, col0 + M) of an M_total-wide subnet. yuma_shard_stage runs
 * stage k of the whole E-epoch run on those columns; between stages the
 * caller combines the per-shard partials of every shard (RCCL all-gather,
 * summed in shard order) and hands the totals back through `io`:
 *
 *   stage 1 -> rowsum_part [E][N][V] = sum over local columns of W
 *   stage 2 <- rowsum      [E][N][V] = sum over shards of rowsum_part
 *           -> csum_part   [E][N]    = sum of local C_raw (fp32; YumaRust:
 *                                      csum_part_d, fp64)
 *   stage 3 <- csum / csum_d [E][N]
 *           -> levels      [E][N][M] quantisation levels of local columns
 *              rsum_part   [E][N]    = sum of local R
 *   stage 4 <- rsum [E][N]; levels_all [E][N][M_total] (liquid scenarios)
 *           -> dsum_part   [E][N][V] = sum over local columns of B * I
 *   stage 5 <- dsum [E][N][V]; writes Dn / D
 * validator_trust (out->Tv, yumas.py:224 `W_clipped.sum(1) / W.sum(1)`):
 *   stage 3 -> tv_part [2][E][N][V] = sums over local columns of Wc and Wn
 *   stage 5 <- tv      [2][E][N][V] = sum over shards of tv_part; Tv = tv[0] / tv[1]
 *   (the workspace must then be sized with full_outputs = 1)
 *
 * Every stage takes the same arguments as yuma_run (W [E][N][V][M] holds the
 * local columns; outputs are the local columns of the [..][M] outputs) and
 * the same workspace, which carries state from stage to stage. params must
 * carry reset_index relative to col0 (reset_mode NONE on shards that do not
 * own the reset column).
 * ---------------------------------------------------------------------- */
typedef struct yuma_shard_io {
  int M_total;             /* global miner count                              */
  int col0;                /* first global column held by this shard          */
  float* rowsum_part;      /* stage 1 out                                     */
  const float* rowsum;     /* stage 2 in                                      */
  float* csum_part;        /* stage 2 out (not YumaRust)                      */
  double* csum_part_d;     /* stage 2 out (YumaRust)                          */
  const float* csum;       /* stage 3, 4 in (not YumaRust)                    */
  const double* csum_d;    /* stage 3, 4 in (YumaRust)                        */
  int* levels;             /* stage 3 out                                     */
  float* rsum_part;        /* stage 3 out                                     */
  const float* rsum;       /* stage 4 in                                      */
  const int* levels_all;   /* stage 4 in, required when a scenario is liquid  */
  float* dsum_part;        /* stage 4 out                                     */
  const float* dsum;       /* stage 5 in                                      */
  float* tv_part;          /* stage 3 out when out->Tv: [2][E][N][V]          */
  const float* tv;         /* stage 5 in when out->Tv:  [2][E][N][V]          */
} yuma_shard_io_t;

int yuma_shard_stage(int stage, int variant, const yuma_params_t* params_dev, int N, int E,
                     int V, int M, const float* W, const float* S, const float* B_init,
                     const float* Wprev_init, const yuma_shard_io_t* io,
                     const yuma_outputs_t* out, void* workspace, size_t workspace_bytes,
                     void* stream);

/* Deterministic synthetic inputs: integer-valued weights whose
 * row sums are exact in fp32. Writes W[e][n][v][m] for epochs t0..t0+E-1.
 * Bit-identical to yuma_simulation._internal.synth.weights (numpy).          */
int yuma_synth_weights(uint64_t seed, int E, int N, int V, int M, int t0, float* W,
                       void* stream);

/* ------------------------------------------------------------------------
 * Weight pairs: the dense uint16 W built on the device.
 *
 * The chain stores a validator's weights as a short list of (uid: u16,
 * weight: u16) pairs, not as a dense row. yuma_weights_from_pairs builds the
 * dense uint16 matrix YUMA_RUN_W_U16 reads from such lists in CSR form: `rows`
 * is E * N * V flattened, so W [rows][M] is the [E][N][V][M] tensor a run
 * takes. Every pointer addresses device memory. The call is stream-ordered,
 * allocates nothing, never synchronises and can be captured into a graph: it
 * is a chain of kernel launches (status zero, fill, scatter, read-back).
 *
 * Row ranges. Row r owns the pairs [row_ptr[r], row_ptr[r + 1]). The host
 * cannot check a list in device memory: the device code clamps the start into
 * [0, nnz] and the end into [start, nnz] before it addresses anything. A row
 * whose range had to be clamped is a bad row: its clamped range is still
 * applied, and it counts once in status[YUMA_PAIRS_ST_BAD_ROWS]. No input
 * makes the engine touch memory outside uid[0 .. nnz), val[0 .. nnz),
 * row_ptr[0 .. rows] or W[0 .. rows * M).
 *
 * Stored values. Every element of W is written; a column no pair names is 0.
 * A pair with uid >= M (a deregistered UID) is dropped and counted in
 * status[YUMA_PAIRS_ST_DROPPED].
 *
 * Duplicates. Two pairs of one row with the same uid and the same weight are
 * harmless. With different weights the element holds one of them, unspecified
 * which, and the row counts once in status[YUMA_PAIRS_ST_CONFLICT_ROWS]. The
 * count is taken by reading the row back after the scatter: a row has a
 * conflict exactly when some in-range pair differs from what its element
 * holds, which is well defined whichever weight won. With status NULL the
 * read-back is not launched.
 *
 * YUMA_PAIRS_UPSCALE: the chain's max-upscale, per row. rowmax is the maximum
 * weight over the row's in-range pairs; the stored value is
 * round_half_even(weight * 65535 / rowmax) in exact integer arithmetic
 * (n = weight * 65535, q = n / rowmax, r = n % rowmax, q + 1 when 2 r > rowmax
 * or when 2 r == rowmax and q is odd): the bits of
 * yuma_simulation's engine.to_u16 (float64 rint) on the densified row. A row
 * whose rowmax is 0 stays 0. A conflict is judged on the raw weights (the
 * scale is at least 1, so different weights of a row store different values).
 *
 * Status: NULL, or YUMA_PAIRS_ST_WORDS 32-bit words. The engine zeroes them
 * itself with a kernel on the stream (not a memset node: a captured call
 * stays a chain of kernel nodes and every replay starts from zero), then adds
 * with vector atomics, modulo 2^32. Word 3 stays 0.
 *
 * Alignment: W, uid and val 2 bytes, status 4, row_ptr 8. The fill stores 16
 * bytes per lane where M % 8 == 0 and W is 16-byte aligned, else 2 bytes; the
 * choice is made on the host from the pointer and M.
 *
 * Refusals, all YUMA_EINVAL, before the first launch and without a HIP call,
 * in this order: rows < 0; M < 1; nnz < 0; a NULL row_ptr, then W, with
 * rows > 0; a NULL uid, then val, with nnz > 0; an unknown flag; rows * M
 * above 2^62 elements (the kernels index W in signed 64 bits; the bound keeps
 * a byte offset and an index one grid stride past the end inside them); a
 * pointer off the alignment above. rows == 0 is then a successful no-op: no
 * launch, status untouched. (No reference counterpart: the reference takes
 * dense float weights only.)
 * ---------------------------------------------------------------------- */
enum yuma_pairs_flags { YUMA_PAIRS_UPSCALE = 1 };
enum {
  YUMA_PAIRS_ST_DROPPED = 0,
  YUMA_PAIRS_ST_CONFLICT_ROWS = 1,
  YUMA_PAIRS_ST_BAD_ROWS = 2,
  YUMA_PAIRS_ST_WORDS = 4
};
int yuma_weights_from_pairs(long long rows, int M, long long nnz,
                            const int64_t* row_ptr,   /* [rows + 1], device */
                            const uint16_t* uid,      /* [nnz], device */
                            const uint16_t* val,      /* [nnz], device */
                            int flags,
                            uint16_t* W,              /* [rows][M], device */
                            uint32_t* status,         /* [YUMA_PAIRS_ST_WORDS], device, or NULL */
                            void* stream);

const char* yuma_last_error(void);
const char* yuma_version(void);
/* Build identity of this library: "src-" + the first 16 hex digits of the
 * SHA-256 of the engine source and this header it was compiled from (stamped
 * by __graft_entry__.build / tools/ab_build.py; "unstamped" otherwise).
 * bench.py pairs a committed counter record with a run only when their build
 * ids match (no reference counterpart: measurement plumbing).               */
const char* yuma_build_id(void);

#ifdef __cplusplus
}
#endif
#endif /* YUMA_HIP_H */
