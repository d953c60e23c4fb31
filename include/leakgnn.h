/*
 * leakgnn.h — C ABI of the MI355X-native GNN message-passing library (libleakgnn.so).
 *
 * This is the drop-in boundary for the hot path of Mateng0228/Leak-det-gnn:
 * the GCN message passing inside models/detector.py::LeakDetector (forward and
 * backward).  The reference has no FFI of its own: its hot path calls PyG
 * (`torch_geometric.nn.GCNConv`, `global_mean_pool`; detector.py:23,162-164,199,215)
 * and plain torch indexing.  Each entry point below names the reference call it
 * replaces (file:line relative to the reference repository root).  The Python
 * binding a maintainer would add on the reference side is shown in INTEGRATION.md.
 *
 * Conventions (all entry points):
 *  - Pointers are DEVICE pointers (caller-owned, e.g. PyTorch caching allocator)
 *    unless the parameter name ends in `_host`.  The library never allocates:
 *    callers pass workspace sized by the matching *_workspace_bytes() query.
 *  - Work is enqueued on `stream` (a hipStream_t; NULL = legacy default stream).
 *    No entry point synchronises the device or the host, so every call is
 *    capturable into a hipGraph.
 *  - Return value: LG_OK (0) or a negative LG_E* code; lg_strerror() names it.
 *    A launch failure returns LG_EHIP.  Compute entry points keep no mutable global
 *    state and are reentrant.  Two OPTIONAL facilities hold state, both documented
 *    at their declarations: the reduce batch (per host thread: begin and flush must
 *    come from the same thread; a flush on another thread returns LG_EINVAL and the
 *    batch stays open on its own thread) and the kernel-timing slots (one process-wide
 *    set of event pairs plus a per-thread armed slot; measurement only).  A caller that
 *    uses neither sees a stateless library.
 *  - Node features are fp32, row-major [B][N][D] (window-major, then node, then
 *    feature; one 4·D-byte row per node).  B identical graphs form the disjoint
 *    union of reference detector.py:105-114; the library keeps ONE single-graph
 *    CSR and offsets rows by b·N itself, so the (2, B·E) batchified edge_index is
 *    never materialised on the hot path.
 *  - Supported feature widths D: 32, 64 (LG_EUNSUPPORTED otherwise).
 *  - Row indices (b·N + n, b·P + p) are 32-bit inside the kernels: B·N and B·P must
 *    be < 2^31 (LG_EUNSUPPORTED otherwise).  Feature tensors larger than 4 GiB are
 *    fine: the GCN entry points split the launch over windows internally.
 */
#ifndef LEAKGNN_H
#define LEAKGNN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* lg_stream_t; /* hipStream_t */

enum {
    LG_OK = 0,
    LG_EINVAL = -1,        /* bad argument (null pointer, negative size, index out of range) */
    LG_EUNSUPPORTED = -2,  /* unsupported feature width / flag combination */
    LG_EHIP = -3           /* HIP launch or runtime error */
};

/* flags for lg_gcn_fwd / lg_gcn_bwd */
#define LG_F_BIAS      0x01  /* fwd: add bias                                                  */
#define LG_F_RELU      0x02  /* fwd: ReLU after bias (F.relu, detector.py:200)                 */
#define LG_F_DROPOUT   0x04  /* fwd: inverted dropout after ReLU (nn.Dropout, detector.py:201) */
#define LG_F_MASK_IN   0x08  /* bwd: dz = dy * scale_in * [y > 0]  (ReLU/dropout backward of THIS layer's output) */
#define LG_F_MASK_OUT  0x10  /* bwd: dx_out = dx * scale_out * [x > 0] (ReLU/dropout backward of the PREVIOUS op) */
/* bwd with node_slot / dnode_bias (ABI 20): rows of dx_out whose node has no sensor
 * (node_slot[n] < 0) MAY be left unwritten; their masked sums are in dnode_bias.  The node
 * init's backward (lg_sensor_proj_bwd) reads only the sensor rows (detector.py:181-186), so
 * layer 0's backward then writes 29 of L-TOWN-A's 661 rows per window instead of all of
 * them.  Honoured by the default node-major schedule of lg_gcn_bwd_nm[_bits]; the other
 * schedules and lg_gcn_bwd write every row. */
#define LG_F_DX_SENSOR_ROWS 0x10000000
/* Node-feature layout for lg_node_init_fwd / lg_pipe_scatter_bwd / lg_edge_head_* /
 * lg_pool_head_fwd: without it node rows are window-major [B][N][D] (row b*N + n, the
 * reference's disjoint-union order, detector.py:105-114, 192-196); with it they are
 * node-major [N][B][D] (row n*B + b), the layout of lg_gcn_fwd_nm / lg_gcn_bwd_nm.
 * Dropout masks are indexed by the window-major row in both layouts. */
#define LG_F_NODE_MAJOR 0x20
/* The bf16 node-MLP tier (BASELINE configs[2], SURVEY §8 d C3: "bf16 for K2/K5/K9 GEMMs
 * with fp32 accumulate"): lg_gcn_fwd_nm / lg_gcn_bwd_nm / lg_edge_head_fwd /
 * lg_edge_head_bwd run their products as ONE bf16 MFMA (operands rounded to bf16, fp32
 * accumulate, fp32 in HBM) instead of the 3-way split that holds fp32 accuracy.  Not an
 * fp32-parity mode: its bar is 2e-2 relative on logits against the fp32 oracle (SURVEY
 * §7).  Ignored by the kernels that have no bf16 form (they compute fp32). */
#define LG_F_BF16 0x40
/* Dropout seeds: every forward entry point taking (seed, salt) reads `seed` as the address
 * of a device-resident uint64 when salt has bit 31 set (the salt proper is bits 0..30).  A
 * captured HIP graph of a training step then re-draws its dropout streams on each replay by
 * refreshing that word on the device, with no host involvement. */
#define LG_SALT_SEED_PTR 0x80000000u
/* lg_gcn_fwd_nm[_bits] kernel and transform.  No bit: the fp32 tier runs the producer /
 * consumer pipeline (k_gcn_fwd_pc: gather waves hand (A x) tiles to MFMA waves through an LDS
 * ring) with the transform as a 2-way fp16 split with power-of-two block scaling (3 f16 MFMAs
 * per product; fp32-level accuracy, ~4e-7 of max |y|); the bf16 tier (LG_F_BF16) the per-wave
 * pipeline k_gcn_fwd_nm3 with ONE bf16 product.
 *   LG_F_BF16X3: the pc pipeline with the 3-way bf16 split (6 bf16 MFMAs per product, ~1e-8 of
 *                max |y|; bit-identical to LG_F_NM3);
 *   LG_F_NM3:    the per-wave pipeline with the 3-way bf16 split;
 *   LG_F_F32_MFMA: the per-wave pipeline on exact v_mfma_f32_16x16x4_f32 (bit-identical to
 *                lg_gcn_fwd on the transposed layout);
 *   LG_F_PC:     with LG_F_BF16: the pc pipeline's single bf16 product. */
#define LG_F_F32_MFMA      0x00400000
#define LG_F_PC            0x00004000
#define LG_F_BF16X3        0x00008000
#define LG_F_NM3           0x00020000

int lg_abi_version(void);

/* Reduce batch (ABI 12).  The backward entry points end in a deterministic slab reduction
 * of their weight/bias gradients (lg_gcn_bwd[_nm], lg_sensor_proj_bwd, lg_edge_head_bwd,
 * lg_pool_head_bwd, lg_gru_bwd, lg_linear_dw).  Between lg_reduce_batch_begin() and
 * lg_reduce_batch_flush(stream) on the SAME host thread those reductions are recorded
 * instead of launched, and the flush launches them together (one launch per 16
 * segments); every gradient column is summed in the same order, so results are unchanged.
 * Until the flush is enqueued the recorded outputs are undefined and the recorded
 * workspaces must stay allocated and unwritten.  A lg_sensor_proj_bwd whose dbias_in is
 * a recorded output folds that output's partials into its own db reduction.  Replaces
 * nothing in the reference: it merges the per-op launches of one backward pass
 * (the autograd of detector.py:170-218).  begin: LG_EINVAL when a batch is already open;
 * flush: LG_EINVAL when none is.  The open batch is THREAD-LOCAL state: a flush from a
 * thread that did not begin it returns LG_EINVAL (nothing launched, the other thread's
 * batch untouched), and a thread that exits with an open batch drops its records. */
int lg_reduce_batch_begin(void);
int lg_reduce_batch_flush(lg_stream_t stream);

/* Measurement helper (bench.py's stream_copy, the achievable-HBM reference beside the
 * 8 TB/s roofline): dst = src over `bytes` (a multiple of 16) with 16-byte non-temporal
 * loads and stores.  No reference counterpart. */
int lg_stream_copy(const void* src, void* dst, int64_t bytes, lg_stream_t stream);

/* Device dropout-seed slots (the seeds LG_SALT_SEED_PTR call sites read at launch): *state
 * += 1, then slots[i] = splitmix64(*state * n + i + 1) & (2^62 - 1), i < n <= 4096, in ONE
 * single-wave launch on the device, so a captured training step re-draws its dropout
 * streams at every replay without the host.  No reference counterpart (the reference's
 * nn.Dropout draws from torch's generator). */
int lg_seed_slots_advance(uint64_t* slots, int64_t n, uint64_t* state, lg_stream_t stream);

/* Replay of a captured step: hipGraphLaunch(graph_exec, stream), n times in a row (graph_exec:
 * an instantiated hipGraphExec_t, e.g. torch.cuda.CUDAGraph.raw_cuda_graph_exec()).  Replaces
 * nothing in the reference (its training step is eager, train_detector.py:296-317). */
int lg_graph_replay(void* graph_exec, int64_t n, lg_stream_t stream);
const char* lg_strerror(int code);

/* Training loss: nn.CrossEntropyLoss() (mean over rows whose target != ignore_index;
 * reference train_detector.py:235, 311) over logits [B][C] (row stride ldx).
 *   fwd: loss (device fp32 scalar), lse [B] (saved for the backward), rowloss [B] scratch;
 *        ONE launch (ABI 23): the rows, and the workgroup that finishes last forms the mean
 *        over rows in row order.  counter: a device uint32, 0 between launches (the launch
 *        resets it); one per stream that may run this concurrently.
 *   bwd: dlogits[b][c] = grad_loss[0] / n * (exp(x - lse[b]) - [c == target[b]]), 0 for
 *        ignored rows (row stride ldd).  Three launches for what torch runs as six.
 *   lse[b] rounds at the size of the logits.  Rows with |lse[b]| >= 32 therefore take the row
 *   loss as (max - x[target]) + log(sum) and the softmax as exp(x - max) / sum, the backward
 *   finding max and sum again; below 32 the rounding is under 1e-6 and the forms above hold.
 *   A target outside [0, C) other than ignore_index (torch raises) gives a NaN loss, reads
 *   nothing out of range, and its dlogits row is the softmax with no one-hot term.  B == 0:
 *   loss = NaN, nothing else written.  Tested against torch's fp64 cross_entropy in
 *   tests/test_gpu_step_tail.py. */
int lg_cross_entropy_fwd(const float* logits, const int64_t* target, int64_t B, int64_t C, int64_t ldx,
                         int64_t ignore_index, float* loss, float* lse, float* rowloss, unsigned* counter,
                         lg_stream_t stream);
int lg_cross_entropy_bwd(const float* logits, const int64_t* target, const float* lse, const float* grad_loss,
                         int64_t B, int64_t C, int64_t ldx, int64_t ignore_index, float* dlogits, int64_t ldd,
                         lg_stream_t stream);

/* The same loss with nn.CrossEntropyLoss's options (added to ABI 26 without a bump: additions
 * only): class weights, label smoothing, the three reductions, and a smoothing table in place
 * of torch's uniform one.  weight: w [C] or NULL (all ones).  smoothing: U [C][C] (row stride
 * ldu >= C) or NULL (every entry 1 / C, torch's label_smoothing); row y is the distribution the
 * eps mass of a row labelled y is spread over.  eps in [0, 1).  reduction: 0 mean, 1 sum, 2 none.
 * For a counted row b (y_b != ignore_index and 0 <= y_b < C):
 *   a_b[c] = w[c] * ((1 - eps) * [c == y_b] + eps * U[y_b][c])
 *   S_b    = sum_c a_b[c]
 *   row_b  = S_b * lse_b - sum_c a_b[c] * x[b][c]            ( = -sum_c a_b[c] * log softmax_b[c] )
 *   mean: loss = sum_b row_b / sum_b w[y_b]     sum: loss = sum_b row_b     none: rowloss[b] = row_b
 *   dlogits[b][c] = G_b * (S_b * softmax_b[c] - a_b[c]),  G_b = grad[0] / sum_b w[y_b] (mean),
 *                   grad[0] (sum), grad[b] (none); exactly 0 for rows that are not counted.
 * A term with a_b[c] == 0 contributes exactly 0, also where x[b][c] = -inf; with a_b[c] > 0 there
 * the loss is +inf, as torch.  Rows with |lse_b| >= 32 take S_b * log(sum) + sum_c a_b[c] *
 * (max - x[b][c]) and exp(x - max) / sum, the rule of lg_cross_entropy_fwd.
 *   fwd: ONE launch.  lse [B], rowsum [B] (S_b) and, for mean and sum, denom (device fp32 scalar,
 *        sum_b w[y_b]) are saved for the backward; rowloss [B] holds row_b (0 for ignored rows)
 *        and is the result for none.  mean / sum: the workgroup that finishes last sums the rows
 *        in row order into loss (device fp32 scalar) and denom and resets counter (as
 *        lg_cross_entropy_fwd's; the two may share one); none: loss, denom and counter are not
 *        used and may be NULL.  No float atomics: bit-identical from run to run.
 *   bwd: ONE launch; grad is a device scalar (mean, sum) or [B] (none); a_b[c] is formed again
 *        from weight, smoothing and eps, which must be those of the forward.
 *   A target outside [0, C) other than ignore_index reads nothing (U is indexed by the label),
 *   gives row_b = NaN (so a NaN mean / sum) and a dlogits row of 0.  B == 0: mean NaN, sum 0,
 *   denom 0, nothing else written.  No row counted: mean NaN (0 / 0, as torch), sum 0.
 *   LG_EINVAL, before any HIP call: B < 0, C <= 0, ldx < C, ldd < C, eps outside [0, 1),
 *   smoothing with ldu < C, reduction outside 0..2, a NULL pointer that the call would use.
 *   Tested against the fp64 expression in tests/test_gpu_ce_options.py. */
int lg_cross_entropy_opt_fwd(const float* logits, const int64_t* target, int64_t B, int64_t C, int64_t ldx,
                             int64_t ignore_index, const float* weight, const float* smoothing, int64_t ldu,
                             float eps, int reduction, float* loss, float* lse, float* rowloss, float* rowsum,
                             float* denom, unsigned* counter, lg_stream_t stream);
int lg_cross_entropy_opt_bwd(const float* logits, const int64_t* target, const float* lse, const float* rowsum,
                             const float* denom, const float* grad, int64_t B, int64_t C, int64_t ldx,
                             int64_t ignore_index, const float* weight, const float* smoothing, int64_t ldu,
                             float eps, int reduction, float* dlogits, int64_t ldd, lg_stream_t stream);

/* Evaluator tails (added to ABI 26 without a bump: additions only).  Both work on rows of logits
 * [.][C] (fp32, row stride ldx >= C) under ONE total order on a row's entries:
 *   a precedes b  <=>  value(a) > value(b), with NaN counted as greater than +inf (torch's argmax
 *                      rule) and -0 equal to +0, or the values are equal and index(a) < index(b).
 * The "first entry" of a row is its argmax with ties (and several NaNs) going to the lowest index;
 * the "position" of an entry is the number of entries that precede it.  On rows with no repeated
 * value and no NaN this is what torch's argmax / topk / argsort compute; on ties, where torch's
 * answer on a GPU is unspecified, it is defined.  C <= 2^31 - 1 (LG_EUNSUPPORTED above).
 *
 * lg_window_metrics: the per-batch tail of DetectorEvaluator.evaluate (reference
 * window_evaluator.py:227-483), ONE launch, one wave per row, each row read once, no sort.
 *   label  : int64 [B].  nlc: the no-leak class, 1 <= nlc <= C - 1.
 *   bucket : int32 [B] or NULL: -1 (none), 0 early, 1 late, 2 pre, 3 noleak.
 *   dist   : fp64 [nlc][nlc] or NULL, dist[y][p] = distance from true pipe y to predicted pipe p.
 *   inv_rank: int32 [nlc][nlc] or NULL (needs dist), inv_rank[p][y] = position of y among p's
 *            neighbours by distance.
 *   radii_host [R], acc_is_host [I]: HOST arrays, R, I in 0 .. LG_WM_MAX_LIST (passed by value to
 *            the launch).
 * Per row with 0 <= label < C:
 *   pred1 = index of the first entry of the row;  hit1 = pred1 == label
 *   hitk  = position of logits[label] among all C entries < min(topk, C)
 *   rank  = 1 + position of logits[min(label, nlc - 1)] among the entries with index < nlc
 *   leak row (label != nlc): missed = pred1 == nlc;  d = missed ? +inf : dist[label][min(pred1, nlc - 1)];
 *                            pos = inv_rank[min(pred1, nlc - 1)][label]
 *     (with C > nlc + 1, a leak label > nlc has no table row: d = +inf and no acc_i, nothing is read)
 * counters: int64 [n_counters], n_counters == LG_WM_COUNTERS, ACCUMULATED in place (the caller
 * zeroes them once), slots in this order:
 *    0 total          1 correct1 (hit1)      2 correctk (hitk)     3 nl_total (label == nlc)
 *    4 nl_correct     5 leak_total           6 leak_correct1       7 leak_correctk
 *    8 tp  9 fp  10 fn  11 tn                (pred1 != nlc  x  label != nlc)
 *   12 + 4 k + {0, 1, 2, 3}: b_total, b_correct1, b_correctk, b_pred_nl (pred1 == nlc) of bucket k
 *   28 pre_false_alarm (label == nlc, pred1 != nlc, bucket 2)       29 noleak_false_alarm (bucket 3)
 *   30 + r: success[r] = leak row and d <= radii[r]                  (untouched without dist)
 *   38 + i: acc_i[i] = leak row, !missed, pos < acc_is[i], acc_is[i] > 0   (untouched without inv_rank)
 *   46 bad_label: a row whose label is outside [0, C) adds here and NOWHERE else; nothing is read
 *      at its label.
 * Integer accumulation only (registers, LDS, then 64-bit integer vector atomics): no float
 * atomics, so the counters do not depend on scheduling and two runs are equal.
 *   rank_out: int32 [B]: rank, 0 on no-leak (and bad-label) rows.
 *   atd_out : fp64 [B], written only with dist: d, NaN on no-leak (and bad-label) rows.
 * LG_EINVAL before any HIP call: B < 0, C < 2, ldx < C, nlc outside 1 .. C - 1, topk < 1, R or I
 * outside 0 .. LG_WM_MAX_LIST (or positive with a NULL host array), inv_rank without dist, NULL
 * counters or n_counters != LG_WM_COUNTERS, and, for B > 0, NULL logits, label, rank_out, or
 * atd_out with dist.  B == 0 returns LG_OK without a launch.
 * Tested against a brute-force statement of the order in tests/test_gpu_window_metrics.py. */
#define LG_WM_MAX_LIST 8
#define LG_WM_COUNTERS 47
int lg_window_metrics(const float* logits, const int64_t* label, int64_t B, int64_t C, int64_t ldx, int64_t nlc,
                      int64_t topk, const int32_t* bucket, const double* dist, const int32_t* inv_rank,
                      const double* radii_host, int R, const int64_t* acc_is_host, int I, int64_t* counters,
                      int64_t n_counters, int32_t* rank_out, double* atd_out, lg_stream_t stream);

/* lg_event_decide: trigger and aggregation of the event evaluator (reference
 * event_evaluator.py:327-342) over the logits [W][C] of one scenario's windows; TWO launches,
 * nothing read back in between.  end_ns: int64 [W], the windows' end times, increasing.
 *   out[0] trig = first row whose first entry (the order above) is not `noleak`; -1 if none
 *   out[1] stop = first i >= trig with end_ns[i] - end_ns[trig] >= agg_ns, W if none, and at
 *                 least trig + 1
 *   summed [C] (or NULL) = logits[trig], then += logits[i] for i = trig + 1 .. stop - 1: each
 *                 column by one thread, in row order, plain fp32 adds
 *   out[2] pred = index of the first entry of that sum
 * Without an alarm out = {-1, -1, -1} and summed is all 0.  workspace: lg_event_decide_workspace_bytes(W)
 * bytes.  LG_EINVAL before any HIP call: W < 0, C < 1, ldx < C, noleak outside [0, C), NULL out, and
 * for W > 0 NULL logits / end_ns / workspace or a workspace that is too small.  W == 0: no alarm. */
int64_t lg_event_decide_workspace_bytes(int64_t W);
int lg_event_decide(const float* logits, const int64_t* end_ns, int64_t W, int64_t C, int64_t ldx, int64_t agg_ns,
                    int64_t noleak, int64_t* out, float* summed, void* workspace, int64_t workspace_bytes,
                    lg_stream_t stream);

/* Training-step tail: torch.nn.utils.clip_grad_norm_(params, max_norm) then
 * torch.optim.AdamW.step() (reference train_detector.py:313-317), ONE launch (ABI 23; two
 * before), two when the parameters need more 1024-element slices than the device has CUs.
 *   table : int64 [T][4] (HOST array) device addresses of (param, grad, exp_avg, exp_avg_sq), fp32
 *   sizes : int64 [T] (HOST array) element counts, T <= 48 (passed by value to the launches, so
 *           captured launches need no host copy)
 *   step  : device fp32 [4] (ABI 25; [2] before): step[0] the AdamW step counter (incremented);
 *           step[1] the launch's workgroup arrival / ticket counter, read as uint32, which must
 *           be 0 between launches (zeros at creation; the launch resets it); step[2] an error
 *           word (uint32, sticky): nonzero when a grid-barrier wait timed out, results invalid;
 *           step[3] reserved
 *   max_norm <= 0: no clipping.  norm_out (device fp32, may be NULL): the pre-clip total norm.
 *   workspace: lg_clip_adamw_workspace_bytes(sizes, T) bytes (ABI 25: one fp64 partial sum of
 *           squares per slice; each workgroup reads and writes only its own gradient slice).
 * The norm is summed in fp64 in a fixed order (deterministic; the one- and two-launch forms
 * give identical bits).  Non-finite gradients behave as torch's pair does (error_if_nonfinite
 * False): a NaN norm gives a NaN clip coefficient, so every clipped gradient and parameter
 * becomes NaN; an infinite norm gives coefficient 0.  eps == 0 with a gradient entry of
 * exactly 0 in a fresh state is 0 / 0: that parameter entry becomes NaN, as in torch's AdamW.
 * T == 0 is legal (the step counter still advances).  Every mode is tested against an fp64
 * AdamW in tests/test_gpu_step_tail.py. */
int64_t lg_clip_adamw_workspace_bytes(const int64_t* sizes, int T);
int lg_clip_adamw(const int64_t* table, const int64_t* sizes, int T, float* step, float lr, float beta1,
                  float beta2, float eps, float weight_decay, float max_norm, float* norm_out, void* workspace, int64_t ws_bytes,
                  lg_stream_t stream);
/* lg_clip_adamw, then (ABI 23) the draw of lg_seed_slots_advance(seed_slots, n_slots, seed_state)
 * in the same launch, by its last workgroup: a captured training step ends by drawing the NEXT
 * replay's dropout seeds, one launch fewer per step. */
int lg_clip_adamw_seeds(const int64_t* table, const int64_t* sizes, int T, float* step, float lr, float beta1,
                        float beta2, float eps, float weight_decay, float max_norm, float* norm_out, void* workspace,
                        int64_t ws_bytes, uint64_t* seed_slots, int64_t n_slots, uint64_t* seed_state,
                        lg_stream_t stream);

/* Hand-off error word (ABI 25; no reference counterpart).  The producer / consumer trunk
 * forward (k_gcn_fwd_pc) bounds every LDS hand-off poll; a poll that runs out sets a bit of a
 * device word (1: producer / W staging, 2: consumer), and that launch's results are invalid.
 * lg_spin_errors copies the word to *out (synchronous, device-wide) and zeroes it if reset. */
int lg_spin_errors(uint32_t* out, int reset);

/* Kernel timing (bench.py; no reference counterpart — the reference has no kernels).
 * lg_timing_arm(slot): the NEXT library kernel launch on this host thread that is the main
 * kernel of an entry point (lg_gcn_fwd[_nm], lg_gcn_bwd[_nm], lg_edge_head_fwd/bwd,
 * lg_gru_fwd/bwd, lg_node_init_fwd, lg_pipe_scatter, lg_pool_head_fwd/bwd, lg_linear_dw,
 * lg_spmm) is launched with hipExtLaunchKernelGGL and the event pair of `slot` (created on
 * first use, reused after; process-wide, so a call on another thread, e.g. autograd's
 * worker, is read back on the caller's): their elapsed time is that kernel's own execution, as a
 * profiler's kernel trace reports it.  lg_timing_disarm returns 1 if the armed pair was
 * never consumed (and drops it), else 0.  lg_timing_elapsed: milliseconds of `slot` once
 * its stop event has completed.  Not for use inside stream capture. */
int lg_timing_arm(int slot);
int lg_timing_disarm(void);
int lg_timing_elapsed(int slot, float* ms);

/* ---------------------------------------------------------------------------
 * K4  gcn_norm + CSR build, once per graph.
 * Replaces: PyG GCNConv.forward -> gcn_norm (add_remaining_self_loops, degree,
 * deg^-1/2, w = dis[src]*dis[dst]) recomputed on every call because the
 * reference constructs GCNConv with cached=False (detector.py:163, 199).
 * Semantics (PyG published algorithm):
 *   add_self_loops: drop existing (i,i) edges, then append (i,i) for every node
 *                   with weight fill_value (1.0; 2.0 for improved=True)
 *   normalize:      deg[d] = sum of weights of edges into d;  dis = deg^-1/2 (inf -> 0);
 *                   w_e = dis[src] * weight_e * dis[dst].     normalize=0 -> w_e = weight_e.
 * Output CSR is keyed by destination (rowptr/col/w) and its transpose keyed by
 * source (rowptr_t/col_t/w_t, used by the backward pass).  Inside each row the
 * entries keep ascending edge order, appended self loop last — the order PyG's
 * scatter_add visits them — so rowptr/col are bit-exact and deterministic.
 *   edge_index : int64 [2][E] device (row 0 = source, row 1 = target)
 *   rowptr, rowptr_t : int32 [N+1];  col, col_t : int32 [E+N];  w, w_t : fp32 [E+N]
 *   rowptr[N] receives the entry count (E minus dropped loops, plus N loops).
 * ------------------------------------------------------------------------- */
int64_t lg_graph_workspace_bytes(int64_t E, int64_t N);
int lg_graph_build(const int64_t* edge_index, int64_t E, int64_t N,
                   int add_self_loops, int normalize, float fill_value,
                   int32_t* rowptr, int32_t* col, float* w,
                   int32_t* rowptr_t, int32_t* col_t, float* w_t,
                   void* workspace, int64_t ws_bytes, lg_stream_t stream);

/* ---------------------------------------------------------------------------
 * Edge weights (PyG GCNConv.forward(x, edge_index, edge_weight): gcn_norm with weights).
 * Added to ABI 26 WITHOUT a version bump: additions only, no existing symbol or signature
 * changed, so a caller built against the earlier 26 keeps working.
 * Semantics (PyG 2.x gcn_norm with edge_weight):
 *   add_self_loops: add_remaining_self_loops: edges with src == dst leave the edge list, one
 *                   loop per node is appended; its weight is fill_value, or, when the input
 *                   held a self-loop edge on that node, that edge's weight (the LAST such
 *                   edge in edge order); earlier self-loop edges of the node are dropped.
 *                   Without add_self_loops nothing is removed or appended.
 *   degree:         deg[d] = weights into d summed in ascending edge order, the appended
 *                   loop last (the order of a CPU index_add_); summed per row after the
 *                   per-row sort, no float atomics, so runs are bit-identical.
 *   normalize:      dis = deg^-1/2 (inf -> 0; each step in fp64, rounded once);
 *                   w = (dis[src] * weight) * dis[dst] in fp32.  normalize = 0: w = weight.
 *   Weights are expected to be non-negative and are not checked: a negative degree gives
 *   NaN, as in PyG.
 * Slot-to-edge map: eid / eid_t (int32, one per CSR slot of the forward / transposed CSR)
 * hold the input edge the slot came from; an appended loop slot holds the self-loop edge
 * that supplied its weight, or -1 when the loop took fill_value.  Every input edge owns at
 * most one slot of each CSR (dropped self loops own none).
 *
 * lg_graph_build_w: lg_graph_build with a device edge_weight (fp32 [E]; may be NULL when
 *   E == 0).  Also writes eid, eid_t (int32 [E+N]) and dis (fp32 [N], kept for the backward).
 * lg_graph_reweight: the structure of an earlier lg_graph_build_w plus a NEW edge_weight:
 *   recomputes dis, w and w_t only (learned weights change every step, edge_index does not).
 *   Kernel launches on `stream` only: no allocation, no host sync, capturable.
 * lg_gcn_norm_bwd: G[k] = dL/dw[k] in forward-CSR order -> dedge_weight = dL/d edge_weight
 *   (fp32 [E]), deterministic, no float atomics: G is routed to the edges through eid (plain
 *   stores), then per node ddis[n] = sum over row n of G v dis[src] + sum over transposed row
 *   n of G v dis[dst] (a loop is in both: its coefficient is v dis[n]^2), ddeg = -1/2 dis^3
 *   ddis, and dv[e] = dis[s] dis[d] G_e + ddeg[d]; the self-loop edge that supplied a loop
 *   weight gets dis[n]^2 G_loop + ddeg[n], dropped edges 0, fill loops nothing.
 *   normalize = 0: dv[e] = G_e.  workspace: lg_gcn_norm_bwd_workspace_bytes (E floats).
 * ------------------------------------------------------------------------- */
int64_t lg_graph_build_w_workspace_bytes(int64_t E, int64_t N);
int lg_graph_build_w(const int64_t* edge_index, const float* edge_weight, int64_t E, int64_t N,
                     int add_self_loops, int normalize, float fill_value,
                     int32_t* rowptr, int32_t* col, float* w, int32_t* eid,
                     int32_t* rowptr_t, int32_t* col_t, float* w_t, int32_t* eid_t, float* dis,
                     void* workspace, int64_t ws_bytes, lg_stream_t stream);
int lg_graph_reweight(const int32_t* rowptr, const int32_t* col, const int32_t* eid,
                      const int32_t* rowptr_t, const int32_t* col_t, const int32_t* eid_t,
                      const float* edge_weight, int64_t E, int64_t N, int normalize, float fill_value,
                      float* dis, float* w, float* w_t, lg_stream_t stream);
int64_t lg_gcn_norm_bwd_workspace_bytes(int64_t E, int64_t N);
int lg_gcn_norm_bwd(const float* G, const int32_t* rowptr, const int32_t* col, const int32_t* eid,
                    const int32_t* rowptr_t, const int32_t* col_t, const int32_t* eid_t,
                    const float* dis, const float* edge_weight, int64_t E, int64_t N, int normalize,
                    float fill_value, float* dedge_weight, void* workspace, int64_t ws_bytes,
                    lg_stream_t stream);

/* Sampled dense-dense product over a CSR: out[k] = sum_c a[row(k)][c] * b[col[k]][c] for
 * every slot k < rowptr[N] (row(k) = the row whose range holds k); elements of out past
 * rowptr[N] stay untouched.  Any C; row strides lda, ldb >= C (floats).  The gradient of a
 * propagate with respect to its coefficients: dL/dw[k] = dy[row k] . x[col k].  One wave
 * walks a row with its a row in registers, the lanes across columns (16-byte loads when C,
 * both strides and both bases allow), several neighbour rows in flight, and a fixed-shape
 * wave reduction: deterministic, no atomics.  32-bit offsets when N * ld fits, else 64-bit.
 * N == 0 or C == 0 returns LG_OK without a launch.  (Added to ABI 26 without a bump.) */
int lg_sddmm_cols(const int32_t* rowptr, const int32_t* col, const float* a, int64_t lda,
                  const float* b, int64_t ldb, float* out, int64_t N, int64_t C, lg_stream_t stream);

/* dL/dw of one node-major GCN layer y = dropout(relu(Ahat x W^T + b)) with respect to the
 * coefficients w[k] of Ahat (learned edge weights on the trunk; x, y, dy : fp32 [N][B][D]):
 *   dz   = LG_F_MASK_IN ? dy * scale * [y > 0] : dy        (lg_gcn_bwd_nm's dz, same flag)
 *   da   = dz W                                             (W : fp32 [D][D], nn.Linear layout)
 *   G[k] = sum_b sum_d da[n][b][d] * x[col[k]][b][d]        for every slot k of row n
 * over the FORWARD CSR rowptr / col of lg_graph_build[_w]; G : fp32 [nnz_cap], slots past
 * rowptr[N] written as 0.  Under LG_F_MASK_IN the mask comes from ymask when non-NULL (the
 * words of lg_gcn_fwd_nm_bits; y may then be NULL), else from y.  One wave per tile (one node
 * x 16 windows x D), the tiles spread over (node, window tile): dz through LDS, da in exact
 * fp32 with W staged once per workgroup, each neighbour block one contiguous 16 x D load, one
 * partial per (tile, slot) from a fixed-shape wave reduction; a second launch adds a slot's
 * partials in ascending tile order in fp64.  No atomics: two runs give the same bits.  Any
 * B >= 1 (rows of a ragged last tile are never read), D in {32, 64}, N*B*D*4 <= 0x7FFFF000
 * (LG_EUNSUPPORTED otherwise).  workspace: lg_sddmm_nm_workspace_bytes(B, nnz_cap) bytes,
 * 16-byte aligned; fewer is LG_EINVAL.  (Added to ABI 26 without a bump.) */
int64_t lg_sddmm_nm_workspace_bytes(int64_t B, int64_t nnz_cap);
int lg_sddmm_nm(const int32_t* rowptr, const int32_t* col, const float* dy, const float* y,
                const uint16_t* ymask, const float* W, const float* x, float* G, int64_t B, int64_t N,
                int64_t D, int64_t nnz_cap, int flags, float scale, void* workspace, int64_t ws_bytes,
                lg_stream_t stream);

/* Node table of the node-major kernels, once per graph (and once for the transposed CSR):
 * one 64-byte record per node = {e0, e1, (col, float_as_int(w)) x 6, self, node} so a tile
 * reads its CSR row with ONE scalar load.  self = position (< 6) of the row's entry whose
 * col is the node itself, -1 if none inline.  Two sections (ABI 13): records 0 .. N-1 in
 * node order, then records N .. 2N-1 in the SCHEDULE order `order` (node order[i] at
 * N + i; NULL = node order), the order in which lg_gcn_fwd_nm / lg_gcn_bwd_nm visit
 * nodes.  The order changes which tiles are in flight together, never a result: with a
 * bandwidth-reducing order (lg_rcm_order) the neighbour rows a tile gathers were gathered
 * by tiles just before it and still sit in L2.
 *   rowptr : int32 [N+1];  pairs : int32 [2 * nnz] (col, float_as_int(w));
 *   order : NULL or device int32 [N], a permutation of 0 .. N-1;
 *   nodetab : int32 [2N][16] (64-byte aligned). */
int lg_nm_table_build(const int32_t* rowptr, const int32_t* pairs, int64_t N, const int32_t* order,
                      int32_t* nodetab, lg_stream_t stream);

/* Sensor marks for the compressed layer-0 input (ABI 21; lg_node_init_bits_fwd /
 * lg_gcn_fwd_nm_x0 / lg_gcn_bwd_nm_x0).  Copies a node table (lg_nm_table_build) and its pair
 * array with every CSR entry whose col n has a sensor slot (node_slot[n] >= 0) rewritten to
 * col = 0x40000000 | node_slot[n], so a tile learns from its record alone which neighbours
 * are stored as sensor rows; pos_slot[i] = node_slot of the schedule section's record N + i.
 *   node_slot : int32 [N] (-1 = no sensor);  nodetab_out : int32 [2N][16];
 *   pairs_out : int32 [2 * nnz];  pos_slot : int32 [N]. */
int lg_nm_table_sensor_mark(const int32_t* nodetab, const int32_t* pairs, int64_t N, int64_t nnz,
                            const int32_t* node_slot, int32_t* nodetab_out, int32_t* pairs_out, int32_t* pos_slot,
                            lg_stream_t stream);

/* Reverse Cuthill-McKee order of the undirected graph edge_index (HOST memory, int64
 * [2][E], self loops and duplicates ignored): order[i] = the node visited i-th.  Each
 * connected component is a breadth-first sweep from a minimum-degree node, neighbours
 * by increasing degree (ties by id), the whole sequence reversed.  Deterministic.  Used as
 * the node-major kernels' schedule order (lg_nm_table_build): on L-TOWN-A it cuts the
 * largest |u - v| over the pipes from 656 to 27.  Returns LG_EINVAL on bad ids. */
int lg_rcm_order(const int64_t* edge_index, int64_t E, int64_t N, int32_t* order);

/* Pipe-endpoint incidence CSR, once per model (backward of detector.py:206-210).
 *   ends : int64 [P][2] device (pipe_ends, utils.py:352-358)
 *   inc_rowptr : int32 [N+1];  inc_item : int32 [2P], item = 2*p + role (role 0 = u, 1 = v),
 *   ascending item order inside each node's row. */
int64_t lg_incidence_workspace_bytes(int64_t P, int64_t N);
int lg_incidence_build(const int64_t* ends, int64_t P, int64_t N,
                       int32_t* inc_rowptr, int32_t* inc_item,
                       void* workspace, int64_t ws_bytes, lg_stream_t stream);

/* K3  disjoint-union edge index (bit-exact).
 * Replaces: detector.py:105-114 `_batchify_edge_index`:  out[:, b*E + e] = ei[:, e] + b*N.
 *   edge_index : int64 [2][E];  out : int64 [2][B*E] */
int lg_batchify_edge_index(const int64_t* edge_index, int64_t E, int64_t N, int64_t B,
                           int64_t* out, lg_stream_t stream);

/* K1+K2  node initialisation (detector.py:178-190) given the sensor projection.
 *   x0[b][n] = dropout(relu(sensor_slot[n] >= 0 ? proj[b][sensor_slot[n]] : bias))
 * where proj[b][s] = h_s[b][s] @ Ws[:, :D]^T + Ws[:, D] + bs is computed by the caller
 * (a 7,424 x 64 x 64 GEMM at B=256) and bias = bs (rows with h0 = 0, mask = 0).
 *   sensor_slot : int32 [N]  (-1 for non-sensor nodes)
 *   proj : fp32 [B][S][D];  bias : fp32 [D];  x0 : fp32 [B][N][D]
 *   flags: LG_F_DROPOUT (p, seed as lg_gcn_fwd; salt distinguishes the call site).  The
 *   keep mask is the row stream of lg_gcn_fwd_nm (seeded per window-major row b*N + n and
 *   lane group), also for lg_node_init_proj_fwd (since ABI 11; the per-element hash before). */
int lg_node_init_fwd(const int32_t* sensor_slot, const float* proj, const float* bias, float* x0,
                     int64_t B, int64_t N, int64_t S, int64_t D,
                     int flags, float dropout_p, uint64_t seed, uint32_t salt, lg_stream_t stream);

/* K1+K2 with the sensor projection folded in: x0 as lg_node_init_fwd with
 *   proj[b][s] = h_s[b][s] @ W[:, :Ds]^T + W[:, Ds] + bias     (W: fp32 [D][Ds+1], nn.Linear layout)
 * formed per sensor row inside the launch (no separate GEMM / proj buffer).
 * sensor_idx: int64 [S], node of sensor s (sensor_slot is its inverse; a duplicated id's
 * earlier entries are skipped, as h0[:, idx] = h_s keeps the last write, detector.py:181).
 * Replaces: sensor_to_node (detector.py:160, 184-189) + node init.  Ds == D in {32, 64}. */
int lg_node_init_proj_fwd(const int32_t* sensor_slot, const int64_t* sensor_idx, const float* h_s, const float* W,
                          const float* bias, float* x0, int64_t B, int64_t N, int64_t S, int64_t Ds, int64_t D,
                          int flags, float dropout_p, uint64_t seed, uint32_t salt, lg_stream_t stream);

/* Backward of the folded projection, from dx0 = the gradient of the node-init
 * pre-activation (lg_gcn_bwd[_nm] of layer 0 with LG_F_MASK_OUT):
 *   dproj[b][s] = dx0[row(sensor_idx[s], b)] * (live ? live[s] : 1)   (row per LG_F_NODE_MAJOR)
 *   dh_s = dproj @ W[:, :Ds];   dW = dproj^T [h_s, 1];   db = sum dproj + dbias_in (may be NULL)
 * live: fp32 [S] (0 for a duplicated sensor id whose row was overwritten, detector.py:181),
 * or NULL.  One launch + one fixed-order slab reduce (deterministic). */
int64_t lg_sensor_proj_bwd_workspace_bytes(int64_t B, int64_t S, int64_t Ds, int64_t D);
int lg_sensor_proj_bwd(const float* dx0, const int64_t* sensor_idx, const float* live, const float* h_s,
                       const float* W, const float* dbias_in, float* dh_s, float* dW, float* db, int64_t B,
                       int64_t N, int64_t S, int64_t Ds, int64_t D, int flags, void* workspace, int64_t ws_bytes,
                       lg_stream_t stream);

/* K2 backward (node init Linear(Ds+1 -> D), detector.py:160, 184-189), weight side:
 * for sensor rows the Linear input is [h_s, 1], so with dy = d(proj) [K][M] (K = B*S rows)
 * and x = h_s [K][N]:
 *   dw[m][n] = sum_k dy[k][m] x[k][n]  (n < N),   dw[m][N] = sum_k dy[k][m]
 *   db[m]    = sum_k dy[k][m]            (db may be NULL)
 * dw is [M][N+1], the nn.Linear weight layout.  M, N in {32, 64}.  Split-K over
 * workgroups, fixed-order reduction (deterministic).  Replaces the skinny-K
 * (K = 7,424) torch.mm of the autograd of torch.addmm. */
int64_t lg_linear_dw_workspace_bytes(int64_t K, int64_t M, int64_t N);
int lg_linear_dw(const float* dy, const float* x, int64_t K, int64_t M, int64_t N,
                 float* dw, float* db, void* workspace, int64_t ws_bytes, lg_stream_t stream);

/* nnz_cap (lg_gcn_fwd / lg_spmm / lg_gcn_bwd): capacity of col/w as allocated for
 * lg_graph_build (E + N).  It sizes the on-chip copy of the CSR: when
 * 4*(N+1) + 8*nnz_cap <= 48 KiB every workgroup stages the CSR in LDS once.
 *
 * K5+K6+K7  fused GCN layer forward (one launch).
 * Replaces: GCNConv.forward (lin -> propagate -> +bias, detector.py:199) and the
 * following F.relu + dropout (detector.py:200-201):
 *   y = dropout(relu( Ahat (x W^T) + b ))  computed as  (Ahat x) W^T + b
 * Each 64-lane wavefront owns 16-row tiles of a persistent, XCD-aware schedule:
 * it gathers a whole tile (CSR segmented reduce in entry order, fp32, 16 lanes per
 * row) into LDS, computes it transposed, y^T = W (Ahat x)^T, on MFMA
 * (v_mfma_f32_16x16x4_f32, exact fp32) while the next tile's row loads are in
 * flight, and applies bias/ReLU/dropout before whole-row stores.
 *   rowptr/col/w : CSR from lg_graph_build;  x, y : fp32 [B][N][D];  W : fp32 [D][D]
 *   (nn.Linear layout [out][in]);  bias : fp32 [D] or NULL.
 *   Dropout: keep element (row, c) iff hash(seed, salt, row*D + c) >= p, scale 1/(1-p).
 *   x and y must not alias. */
int lg_gcn_fwd(const int32_t* rowptr, const int32_t* col, const float* w,
               const float* x, const float* W, const float* bias, float* y,
               int64_t B, int64_t N, int64_t D, int64_t nnz_cap,
               int flags, float dropout_p, uint64_t seed, uint32_t salt, lg_stream_t stream);

/* Node-major fused GCN layer (LG_F_NODE_MAJOR layout, x, y : fp32 [N][B][D]).
 * Same math, flags and results as lg_gcn_fwd on the transposed layout: rows n*B + b.
 * Every window shares the graph, so a 16-row tile is one node and 16 consecutive
 * windows, and each CSR entry (m, w) names one contiguous 16 x D block of x — the
 * entry is wave-uniform and the row loads need no per-lane index arithmetic.
 *   nodetab : int32 [2N][16] from lg_nm_table_build (one 64-byte record per node:
 *             e0, e1, the first 6 (col, w) pairs of the row, self position, node id;
 *             tiles are visited in the table's schedule order);
 *   pairs : int32 [2 * nnz] interleaved (col, float_as_int(w)) of the lg_graph_build CSR.
 *   Dropout: row-stream masks indexed by the window-major row b*N + n (the mask of
 *   lg_gcn_fwd for the same seed/salt).
 *   Requires N*B*D*4 <= 0x7FFFF000 bytes (LG_EUNSUPPORTED otherwise; callers split
 *   larger batches over windows). */
int lg_gcn_fwd_nm(const int32_t* nodetab, const int32_t* pairs, const float* x, const float* W,
                  const float* bias, float* y, int64_t B, int64_t N, int64_t D, int64_t nnz_cap,
                  int flags, float dropout_p, uint64_t seed, uint32_t salt, lg_stream_t stream);
/* Backward of lg_gcn_fwd_nm: lg_gcn_bwd's contract on the node-major layout, over the
 * transposed CSR given as nodetab_t (lg_nm_table_build of rowptr_t) + pairs_t.
 * workspace: lg_gcn_bwd_nm_workspace_bytes(D). */
int64_t lg_gcn_bwd_nm_workspace_bytes(int64_t D);
int lg_gcn_bwd_nm(const int32_t* nodetab_t, const int32_t* pairs_t, const float* dy, const float* y,
                  const float* x, const float* W, float* dx_out, float* dW, float* db,
                  const int32_t* node_slot, float* dnode_bias, int64_t B, int64_t N, int64_t D,
                  int flags, float scale_in, float scale_out, void* workspace, int64_t ws_bytes, lg_stream_t stream);

/* The layer's output mask as bits (ABI 15).  lg_gcn_fwd_nm_bits = lg_gcn_fwd_nm that also
 * writes ymask (when non-NULL): [y > 0] of every output element, one uint16 per lane and
 * 16-row tile (node n, window group g = b / 16): bit 4k + i of lane l at
 * ((n * ceil(B/16) + g) * 64 + l) * 2 bytes is row g*16 + (64/(D/4)) k + l / (D/4), channel
 * 4 (l % (D/4)) + i  ->  N * ceil(B/16) * 128 bytes (1/32 of y).  lg_gcn_bwd_nm_bits =
 * lg_gcn_bwd_nm that, under LG_F_MASK_IN with ymask non-NULL, reads the mask from those
 * bits instead of gathering y (y may then be NULL).  Same results as the y path. */
/* The fp32-tier forward transform: see the LG_F_PC / LG_F_BF16X3 / LG_F_NM3 flags above. */
int lg_gcn_fwd_nm_bits(const int32_t* nodetab, const int32_t* pairs, const float* x, const float* W,
                       const float* bias, float* y, int64_t B, int64_t N, int64_t D, int64_t nnz_cap,
                       int flags, float dropout_p, uint64_t seed, uint32_t salt, lg_stream_t stream,
                       uint16_t* ymask);
/* lg_gcn_bwd_nm[_bits] transform (ABI 22): on the fp32 tier both GEMMs (dx^T = W^T t^T,
 * dW = t^T x) run on the 2-way fp16 split with power-of-two scales — W^T per workgroup, each
 * 16-row tile's t and x blocks per tile — (|err| ~1e-7 of scale); LG_F_BF16X3 restores the
 * 3-way bf16 split (~1e-8).  Measured equal in time at B = 256 (the kernel is bound by its
 * gathers, not the transform); LG_F_BF16: one bf16 product. */
int lg_gcn_bwd_nm_bits(const int32_t* nodetab_t, const int32_t* pairs_t, const float* dy, const float* y,
                       const float* x, const float* W, float* dx_out, float* dW, float* db,
                       const int32_t* node_slot, float* dnode_bias, int64_t B, int64_t N, int64_t D,
                       int flags, float scale_in, float scale_out, void* workspace, int64_t ws_bytes, lg_stream_t stream,
                       const uint16_t* ymask);

/* Residual (identity-skip) layer, x_out = x + f(x) with f = dropout(relu(Ahat x W^T + b))
 * (added to ABI 26 without a bump: additions only).  A deep trunk is trained with identity
 * skips; the plain backward recovers a layer's ReLU/dropout mask as [y > 0], which is wrong
 * once y = x + f, so both calls carry the branch's own mask as bits.
 * lg_gcn_fwd_nm_skip: lg_gcn_fwd_nm_bits' arguments; ymask is required (LG_EINVAL).
 *   y = x_own + f, where f is exactly lg_gcn_fwd_nm_bits' y for the same arguments and ymask
 *   holds [f > 0] (NOT [y > 0]), bit for bit that call's ymask.  The sum is one fp32 add per
 *   element, the last operation before the store.  x and y must not alias.  Runs on the
 *   producer / consumer kernel of the fp32 tier only (the f16x2 transform, or LG_F_BF16X3):
 *   LG_F_BF16, LG_F_NM3 and LG_F_F32_MFMA return LG_EUNSUPPORTED.
 * lg_gcn_bwd_nm_skip: lg_gcn_bwd_nm_bits' arguments; LG_F_MASK_IN and ymask (the forward's
 *   [f > 0] bits) are required (LG_EINVAL), LG_F_BF16 returns LG_EUNSUPPORTED.  With
 *   dz = dy * scale_in * mask:  t = Ahat^T dz, dW and db exactly as lg_gcn_bwd_nm_bits';
 *   dx = t W + dy_own (one fp32 add after the product); then LG_F_MASK_OUT as there:
 *   dx_out = (t W + dy) * scale_out * [x > 0].  LG_F_DX_SENSOR_ROWS and dnode_bias keep their
 *   meaning on the summed dx (dnode_bias is summed in another, still fixed, order than
 *   lg_gcn_bwd_nm_bits').  dy and dx_out must not alias. */
int lg_gcn_fwd_nm_skip(const int32_t* nodetab, const int32_t* pairs, const float* x, const float* W,
                       const float* bias, float* y, int64_t B, int64_t N, int64_t D, int64_t nnz_cap,
                       int flags, float dropout_p, uint64_t seed, uint32_t salt, lg_stream_t stream,
                       uint16_t* ymask);
int lg_gcn_bwd_nm_skip(const int32_t* nodetab_t, const int32_t* pairs_t, const float* dy, const float* y,
                       const float* x, const float* W, float* dx_out, float* dW, float* db,
                       const int32_t* node_slot, float* dnode_bias, int64_t B, int64_t N, int64_t D,
                       int flags, float scale_in, float scale_out, void* workspace, int64_t ws_bytes, lg_stream_t stream,
                       const uint16_t* ymask);

/* LayerNorm over the feature axis, for the pre-norm residual trunk (added to ABI 26 without a
 * bump: additions only):  xn_l = LN_l(x_l),  f_l = dropout(relu(Ahat xn_l W_l^T + b_l)),
 * x_{l+1} = x_l + f_l.  The branch runs on lg_gcn_fwd_nm_bits / lg_gcn_bwd_nm_bits unchanged (their
 * input may be signed); the add of the skip and the norm in front of the next branch are one
 * launch here.  Rows are D contiguous floats (rows = N * B in either layout), D in {32, 64}
 * (LG_EUNSUPPORTED otherwise), rows < 2^31.  wave64, one row per D/4 lanes, 16-byte loads and
 * stores, no atomics; every result is bit-reproducible from run to run.
 * lg_add_layernorm_fwd:
 *   xsum = x + f                       one fp32 add per element; f and xsum both NULL: xsum is x
 *                                      (the entry norm of x_0); one without the other: LG_EINVAL
 *   mean = sum(xsum) / D,  var = sum((xsum - mean)^2) / D      two passes over the row in
 *                                      registers, never E[x^2] - mean^2 (the stream grows with depth)
 *   rstd = 1 / sqrt(var + eps)
 *   xn   = (xsum - mean) * rstd * gamma + beta
 *   stats [rows][2] = (mean, rstd), or NULL (inference).  x, xn, gamma, beta NULL, rows < 0 or
 *   eps < 0: LG_EINVAL.  No output may alias an input.
 * lg_layernorm_bwd: x is the forward's xsum, stats its (mean, rstd).  With xhat = (x - mean) * rstd,
 *   g = dxn * gamma:
 *   dx     = rstd * (g - mean(g) - xhat * mean(g * xhat))
 *   dx     = dx + carry                when carry is non-NULL: one fp32 add (the gradient that
 *                                      reaches x_l past the norm, through the skip)
 *   dx_out = LG_F_MASK_OUT ? dx * scale_out * [x > 0] : dx     (the node init's ReLU / dropout
 *                                      backward at the entry norm; the last arithmetic)
 *   dgamma = sum_rows dxn * xhat,  dbeta = sum_rows dxn: per-workgroup partials in the workspace,
 *   then the fixed-order slab reduction (inside an open reduce batch: recorded for its launch).
 *   dx_out may alias no input.  flags other than LG_F_MASK_OUT: LG_EUNSUPPORTED.  workspace:
 *   lg_layernorm_bwd_workspace_bytes(D) bytes, 16-byte aligned; NULL or fewer is LG_EINVAL, as is
 *   a NULL dxn, x, stats, gamma, dx_out, dgamma or dbeta.  rows == 0 writes zeros to dgamma, dbeta. */
int lg_add_layernorm_fwd(const float* x, const float* f, const float* gamma, const float* beta, float* xsum,
                         float* xn, float* stats, int64_t rows, int64_t D, float eps, lg_stream_t stream);
int64_t lg_layernorm_bwd_workspace_bytes(int64_t D);
int lg_layernorm_bwd(const float* dxn, const float* x, const float* stats, const float* gamma, const float* carry,
                     float* dx_out, float* dgamma, float* dbeta, int64_t rows, int64_t D, int flags, float scale_out,
                     void* workspace, int64_t ws_bytes, lg_stream_t stream);

/* K-hop diffusion of the node init (APPNP's personalised-PageRank propagation; csrc/diffuse.hip;
 * added to ABI 26 without a bump: additions only).  Node-major x0, z, g, dx0 : fp32 [N][B][D], D in
 * {32, 64} (LG_EUNSUPPORTED otherwise).  Ahat comes from the node tables of lg_nm_table_build (records
 * 0 .. N-1; self loop and edge weights included): nodetab / pairs forward, nodetab_t / pairs_t backward.
 *   lg_diffuse_fwd:  z_0 = x0,  z_{k+1} = (1 - alpha) Ahat z_k + alpha x0,  z_out = z_hops
 *   lg_diffuse_bwd:  u = g, acc = 0;  hops times: acc += alpha u, u = (1 - alpha) Ahat^T u;
 *                    dx0 = u + acc;  dx0_out = LG_F_MASK_OUT ? dx0 * scale_out * [x0 > 0] : dx0
 *                    (the node init's ReLU / dropout mask, the last arithmetic, as lg_layernorm_bwd's;
 *                    x0 may be NULL without the flag, LG_EINVAL with it)
 * Two forms of each pass, the same bits from both (a row's entries are summed in the record's CSR
 * order, inline pairs then overflow pairs, with the same unfused fp32 operations):
 *   resident: ONE launch runs every hop; a workgroup owns one window and a channel slice of 32, 16 or
 *     8 floats whose N rows stay in LDS (lg_diffuse_slice(N, D): the widest slice whose rows fit the
 *     160 KiB of LDS and 12 rows in each of 512 threads' registers, i.e. N <= 768, 1536, 3072; 0: none).  x0 is read once, z_out written
 *     once.  No atomics, no cross-workgroup hand-off.  Needs no workspace.
 *   hop-wise: one launch per hop, ping-pong between the output and the workspace, any N.  Taken when
 *     no slice fits, or under LG_F_DIFFUSE_HOPWISE (tests, measurement).
 * workspace: lg_diffuse_workspace_bytes(B, N, D, hops, flags, backward) bytes, 16-byte aligned (0 for
 * the resident form and for hops == 1: NULL is then accepted); fewer is LG_EINVAL.
 * LG_EINVAL: a NULL table, input or output, B < 0, N <= 0, hops outside 1 .. 64, alpha outside [0, 1]
 * (NaN included), the output aliasing the input (x0 == z_out, g == dx0_out, x0 == dx0_out under the
 * mask).  Other flags: LG_EUNSUPPORTED, as is N * B >= 2^31.  B == 0 returns LG_OK without a launch. */
#define LG_F_DIFFUSE_HOPWISE 0x100
int lg_diffuse_slice(int64_t N, int64_t D);
int64_t lg_diffuse_workspace_bytes(int64_t B, int64_t N, int64_t D, int64_t hops, int flags, int backward);
int lg_diffuse_fwd(const int32_t* nodetab, const int32_t* pairs, const float* x0, float* z_out, int64_t B, int64_t N,
                   int64_t D, int64_t hops, float alpha, int flags, void* workspace, int64_t ws_bytes,
                   lg_stream_t stream);
int lg_diffuse_bwd(const int32_t* nodetab_t, const int32_t* pairs_t, const float* g, const float* x0, float* dx0_out,
                   int64_t B, int64_t N, int64_t D, int64_t hops, float alpha, int flags, float scale_out,
                   void* workspace, int64_t ws_bytes, lg_stream_t stream);

/* Compressed layer-0 input (ABI 21).  The node init's non-sensor rows are dropout(relu(b)):
 * 632 of L-TOWN-A's 661 rows carry no information beyond their keep bits, yet materialising
 * x0 costs a 43 MB write and layer 0's forward and backward read it back (86 MB).
 * lg_node_init_bits_fwd replaces lg_node_init_proj_fwd (LG_F_NODE_MAJOR layout) with
 *   xs0    : fp32 [S][B][D], x0's rows of the live sensor slots (node_slot[n] = s), bit-identical
 *            to lg_node_init_proj_fwd's rows;
 *   x0bits : uint16 [N * ceil(B/16) * 64], [x0 > 0] of EVERY row in the mask layout of
 *            lg_gcn_fwd_nm_bits (ABI 15),
 * from which a non-sensor element is x0 = bit ? relu(bias) * scale : 0 exactly.
 * lg_gcn_fwd_nm_x0 is lg_gcn_fwd_nm_bits of layer 0 reading (xs0, x0bits, node_bias) through a
 * sensor-marked node table (lg_nm_table_sensor_mark): the gather waves read one 2-byte mask word
 * per neighbour block and the transform waves add the sensor neighbours' xs0 rows (ABI 22), so
 * y equals the dense forward up to that summation order (~1e-7 of scale).  lg_gcn_bwd_nm_x0 is lg_gcn_bwd_nm_bits of layer 0 (no
 * MASK_IN) with the tile's own x block from (xs0, x0bits); pos_slot_t = the transposed table's
 * schedule-section slots.  The node init and the layer share one Dropout (detector.py:190,
 * 201): flags' LG_F_DROPOUT and dropout_p describe both.  lg_node_init_expand materialises x0
 * (diagnostics, tests).  lg_gcn_fwd_nm_x0 runs on the producer / consumer kernel only: LG_F_NM3
 * and LG_F_F32_MFMA return LG_EUNSUPPORTED (ABI 25; ignored before). */
int lg_node_init_bits_fwd(const int32_t* sensor_slot, const int64_t* sensor_idx, const float* h_s, const float* W,
                          const float* bias, float* xs0, uint16_t* x0bits, int64_t B, int64_t N, int64_t S,
                          int64_t Ds, int64_t D, int flags, float dropout_p, uint64_t seed, uint32_t salt,
                          lg_stream_t stream);
int lg_node_init_expand(const int32_t* sensor_slot, const float* xs0, const uint16_t* x0bits, const float* bias,
                        float* x0, int64_t B, int64_t N, int64_t D, int flags, float dropout_p, lg_stream_t stream);
int lg_gcn_fwd_nm_x0(const int32_t* nodetab_s, const int32_t* pairs_s, const float* xs0, const uint16_t* x0bits,
                     const float* node_bias, const float* W, const float* bias, float* y, int64_t B, int64_t N,
                     int64_t S, int64_t D, int flags, float dropout_p, uint64_t seed, uint32_t salt,
                     lg_stream_t stream);
int lg_gcn_bwd_nm_x0(const int32_t* nodetab_t, const int32_t* pairs_t, const int32_t* pos_slot_t, const float* dy,
                     const float* xs0, const uint16_t* x0bits, const float* node_bias, const float* W, float* dx_out,
                     float* dW, float* db, const int32_t* node_slot, float* dnode_bias, int64_t B, int64_t N,
                     int64_t S, int64_t D, int flags, float dropout_p, float scale_out, void* workspace,
                     int64_t ws_bytes, lg_stream_t stream);

/* Single graph (B = 1) on the node tables (ABI 18): the GCNConv module's own call shape,
 * x [N][D] (BASELINE configs[4], one 100k-node graph).  Replaces: PyG GCNConv.forward
 * (detector.py:163,199 — lin, propagate, bias) and its autograd backward for ONE graph.
 * Tiles of 16 nodes in the table's schedule order; transform and dx on the 3-way bf16
 * split (fp32-level, ~1e-7 of scale), not bit-identical to lg_gcn_fwd / lg_gcn_bwd.
 *   lg_gcn_fwd_rows: y = Ahat x W^T (+ b with LG_F_BIAS; no other flags).
 *   lg_gcn_bwd_rows: t = Ahat^T dy; dx = t W; dW = t^T x; db = sum_rows dy (db may be NULL);
 *     workspace lg_gcn_bwd_nm_workspace_bytes(D).
 * D = 64 only (LG_EUNSUPPORTED otherwise: use lg_gcn_fwd / lg_gcn_bwd). */
int lg_gcn_fwd_rows(const int32_t* nodetab, const int32_t* pairs, const float* x, const float* W, const float* bias,
                    float* y, int64_t N, int64_t D, int flags, lg_stream_t stream);
int lg_gcn_bwd_rows(const int32_t* nodetab_t, const int32_t* pairs_t, const float* dy, const float* x,
                    const float* W, float* dx, float* dW, float* db, int64_t N, int64_t D, void* workspace, int64_t ws_bytes,
                    lg_stream_t stream);

/* Plain propagate y = Ahat x (PyG MessagePassing.propagate with the gcn_norm
 * weights; no transform).  Used for the HBM-roofline stress case (config C5). */
int lg_spmm(const int32_t* rowptr, const int32_t* col, const float* w,
            const float* x, float* y, int64_t B, int64_t N, int64_t D, int64_t nnz_cap, lg_stream_t stream);

/* Propagate of any width: y[n][c] = sum over row n of the CSR (entry order) of
 * w[e] x[col[e]][c], plus bias[c] when bias is non-null, for n < N, c < C (row strides ldx,
 * ldy >= C, in floats; x and y must not alias).  The general path of GCNConv (in_channels !=
 * out_channels or widths other than 32 / 64: reference detector.py:198-199 builds
 * GCNConv(hidden, hidden), PyG's GCNConv takes any pair): y = Ahat (x W^T) + b with the
 * transform on a library GEMM, or (x's width < the output's) (Ahat x) W^T + b; the backward is
 * the same call over the transposed CSR (lg_graph_build's rowptr_t / col_t / w_t).  No
 * capacity limits beyond N * C < 2^62.  (ABI 24) */
int lg_spmm_cols(const int32_t* rowptr, const int32_t* col, const float* w, const float* x, int64_t ldx,
                 const float* bias, float* y, int64_t ldy, int64_t N, int64_t C, lg_stream_t stream);

/* Fused GCN layer backward (one main launch + one deterministic slab reduction).
 * Given dy = dL/dy of this layer's output:
 *   dz     = LG_F_MASK_IN ? dy * scale_in * [y > 0] : dy
 *   t      = Ahat^T dz                     (gather over the transposed CSR)
 *   dx     = t W                           (MFMA)
 *   dW     = t^T x                         (MFMA, per-block fp32 slabs, fixed-order reduce)
 *   db     = sum_rows dz
 *   dx_out = LG_F_MASK_OUT ? dx * scale_out * [x > 0] : dx
 * Replaces: the autograd backward of GCNConv (lin, propagate, bias) and of the
 * relu/dropout pairs around it (detector.py:189-190, 198-201).
 *   dnode_bias = sum over rows b*N + n with node_slot[n] < 0 of dx_out
 *              (the node-init bias gradient, detector.py:184-190: rows without a
 *              sensor are relu(bias)); node_slot / dnode_bias both NULL to skip.
 *   y may be NULL unless LG_F_MASK_IN;  db may be NULL.
 *   workspace : lg_gcn_bwd_workspace_bytes(D) bytes. */
int64_t lg_gcn_bwd_workspace_bytes(int64_t D);
int lg_gcn_bwd(const int32_t* rowptr_t, const int32_t* col_t, const float* w_t,
               const float* dy, const float* y, const float* x, const float* W,
               float* dx_out, float* dW, float* db,
               const int32_t* node_slot, float* dnode_bias,
               int64_t B, int64_t N, int64_t D, int64_t nnz_cap,
               int flags, float scale_in, float scale_out,
               void* workspace, int64_t ws_bytes, lg_stream_t stream);

/* K8 forward: per-pipe endpoint gather + EdgeHead feature build.
 * Replaces: detector.py:206-210 and :87  feat = cat[h_u, h_v, |h_u - h_v|].
 *   ends : int64 [P][2];  h : fp32 [B][N][D];  feat : fp32 [B][P][3D] */
int lg_pipe_gather_fwd(const int64_t* ends, const float* h, float* feat,
                       int64_t B, int64_t N, int64_t P, int64_t D, lg_stream_t stream);

/* K8 backward + K10 backward, fused: deterministic segmented reduce over the
 * incidence CSR (no atomics):
 *   dh[b][n] = dpool[b]/N + sum over incidences (p, role) of n, in item order, of dpipe[b][p][role]
 * where dpipe[b][p][0] / [1] are the gradients w.r.t. h_u / h_v of pipe p (from
 * lg_edge_head_bwd).  dpool may be NULL.
 * Replaces: autograd of h_nodes[:, u], h_nodes[:, v] (detector.py:209-210) and of
 * global_mean_pool (detector.py:215).   dpipe : fp32 [B][P][2][D];  dh : fp32 [B][N][D] */
int lg_pipe_scatter_bwd(const int32_t* inc_rowptr, const int32_t* inc_item, const float* dpipe,
                        const float* dpool, float* dh,
                        int64_t B, int64_t N, int64_t P, int64_t D, int flags, lg_stream_t stream);

/* K8 + K9 fused EdgeHead forward (detector.py:76-88 applied at :206-211):
 *   logits[b][p] = W2 . dropout(relu(W1 [h_u, h_v, |h_u - h_v|] + b1)) + b2
 * feat (B,P,3D) and the hidden layer are never materialised.  W1 : fp32 [hidden][3D]
 * (edge_head.mlp.0.weight), b1 [hidden], W2 [hidden] (mlp.3.weight), b2 [1];
 * logits : fp32, element (b, p) at logits[b*ldo + p] (ldo >= P; ldo = P+1 writes the
 * pipe columns of detector.py:216's (B, P+1) output in place).  hidden must be 128;
 * D in {32, 64}.  Dropout as lg_gcn_fwd, index (b*P + p)*hidden + unit.
 * hid: NULL, or fp32 [B*P][hidden] receiving the post-dropout hidden layer (what
 * lg_edge_head_bwd needs; pass it in training).  The products run on f16 MFMA with
 * 2-way split, power-of-two-scaled fp32 operands (D = 64, fp32 tier; W1 scaled per wave,
 * the features per pipe row, dropped term <= 2^-22 of each product) or, with
 * LG_F_BF16X3 and at D = 32, on bf16 MFMA with 3-way split operands: fp32-level
 * accuracy either way, not bit-identical to an fp32 GEMM.  LG_F_BF16: bf16 hi parts only. */
int lg_edge_head_fwd(const int64_t* ends, const float* h, const float* w1, const float* b1,
                     const float* w2, const float* b2, float* logits, int64_t ldo, float* hid,
                     int64_t B, int64_t N, int64_t P, int64_t D, int64_t hidden,
                     int flags, float dropout_p, uint64_t seed, uint32_t salt, lg_stream_t stream);
/* Backward of lg_edge_head_fwd: hid (its hidden-layer output) and dlogits (row stride
 * ldo) -> dpipe fp32 [B][P][2][D] (grads w.r.t. h_u, h_v per pipe), dw1/db1/dw2/db2
 * (overwritten; deterministic fixed-order reduction of per-workgroup slabs).  flags and
 * dropout_p as in the forward (the keep mask is read back as [hid > 0]).  Transform (ABI
 * 22): on the fp32 tier the f16x2 split — g rows scaled per pipe row from |dlogit| (dpipe
 * independent of which rows share a tile), W1^T per wave, dW1's products per tile (features
 * scaled by 2^(T - sg(row))); LG_F_BF16X3: the 3-way bf16 split; LG_F_BF16: one product. */
int64_t lg_edge_head_bwd_workspace_bytes(int64_t B, int64_t P, int64_t D, int64_t hidden);
int lg_edge_head_bwd(const int64_t* ends, const float* h, const float* w1, const float* w2,
                     const float* hid, const float* dlogits, int64_t ldo, float* dpipe,
                     float* dw1, float* db1, float* dw2, float* db2,
                     int64_t B, int64_t N, int64_t P, int64_t D, int64_t hidden,
                     int flags, float dropout_p, void* workspace, int64_t ws_bytes, lg_stream_t stream);
/* lg_edge_head_bwd followed by lg_pipe_scatter_bwd (dh = dpool / N + the incidence sums of
 * dpipe; reference detector.py:206-211 and the backward of its gather), fused into the
 * backward kernel.  With a pipe schedule (sched: device copy of lg_pipe_schedule_build's
 * buffer, sched_hdr: its first 16 words in HOST memory; ABI 22) the node sums are STREAMED:
 * pipes are visited in the schedule's order, each tile's per-pipe rows stay in LDS and are
 * added to the running sums of the nodes they touch (LDS slots for the nodes still open, the
 * dh row at a node's last tile) — dpipe is neither written nor read.  The sums are those of
 * lg_pipe_scatter_bwd over the schedule's incidence CSR (inc_rowptr / inc_item from the same
 * build), bit for bit.  Without a schedule (NULL, NULL), or when the open sums do not fit in
 * LDS, each workgroup owns whole windows and sums a window's node rows from its just-written
 * dpipe rows (ABI 19; the CSR staged in LDS), or, when the CSR does not fit either, the two
 * calls run.  Both fused forms run one workgroup per window, so with fewer windows (B) than
 * CUs the two calls run instead.  dpipe: scratch [B][P][2][D] (untouched by the streamed path); dpool: NULL or
 * [B][D] (lg_pool_head_bwd's dpooled, computed before this call); the workspace is
 * lg_edge_head_bwd_workspace_bytes.  A schedule for another (P, N, D) is LG_EINVAL. */
int lg_edge_head_bwd_scatter(const int64_t* ends, const float* h, const float* w1, const float* w2,
                             const float* hid, const float* dlogits, int64_t ldo, float* dpipe,
                             float* dw1, float* db1, float* dw2, float* db2, const int32_t* inc_rowptr,
                             const int32_t* inc_item, const int32_t* sched, const int32_t* sched_hdr,
                             const float* dpool, float* dh,
                             int64_t B, int64_t N, int64_t P, int64_t D, int64_t hidden,
                             int flags, float dropout_p, void* workspace, int64_t ws_bytes, lg_stream_t stream);

/* Both heads' backward (ABI 23): lg_pool_head_bwd (the NoLeakHead, first argument block) then
 * lg_edge_head_bwd_scatter, as ONE launch when the streamed form applies (a pipe schedule, a
 * window per workgroup): the NoLeakHead backward of each workgroup's windows runs in its
 * prologue (the same sums in the same order as k_pool_head_bwd), dpool [B][D] becomes a scratch
 * the launch writes and reads back.  Otherwise the two calls, in that order (dpool their
 * hand-off).  nworkspace: lg_pool_head_bwd_workspace_bytes; workspace:
 * lg_edge_head_bwd_workspace_bytes.  Replaces detector.py:214-216's and :206-211's autograd
 * (global_mean_pool + NoLeakHead, pipe gather + EdgeHead). */
int lg_heads_bwd_scatter(const float* pooled, const float* nhid, const float* nw1, const float* nw2, float* ndw1,
                         float* ndb1, float* ndw2, float* ndb2, int nflags, float n_dropout_p, void* nworkspace,
                         int64_t nws_bytes, const int64_t* ends, const float* h, const float* w1, const float* w2,
                         const float* hid, const float* dlogits, int64_t ldo, float* dpipe, float* dw1, float* db1,
                         float* dw2, float* db2, const int32_t* inc_rowptr, const int32_t* inc_item,
                         const int32_t* sched, const int32_t* sched_hdr, float* dpool, float* dh, int64_t B, int64_t N,
                         int64_t P, int64_t D, int64_t hidden, int flags, float dropout_p, void* workspace,
                         int64_t ws_bytes, lg_stream_t stream);

/* Pipe schedule of the streamed EdgeHead backward (ABI 22), once per model; HOST memory in and
 * out (upload sched to the device; keep its first 16 words on the host as sched_hdr).
 *   ends : int64 [P][2];  D : 32 or 64 (the tile height 2048 / D);
 *   sched : int32 [words] with words >= lg_pipe_schedule_words(P, N, D);
 *   inc_rowptr [N+1], inc_item [2P]: the incidence CSR (as lg_incidence_build) with each node's
 *     items in SCHEDULE order instead of ascending — pass it to lg_pipe_scatter_bwd /
 *     lg_edge_head_bwd_scatter with this schedule, so every path sums in one order.
 * Pipes are ordered by their endpoints' positions in lg_rcm_order of the pipe graph (the later
 * one first, then the earlier, then the id); a node is "open" from its first tile to its last.
 * Header words: version, P, N, D, TR, tiles, open slots, max events per tile, block words,
 * nodes without pipes, the three section offsets, total words.  Deterministic.
 * LG_EUNSUPPORTED when N >= 2^24. */
#define LG_PIPE_SCHED_VERSION 1
int64_t lg_pipe_schedule_words(int64_t P, int64_t N, int64_t D);
int lg_pipe_schedule_build(const int64_t* ends, int64_t P, int64_t N, int64_t D, int32_t* sched, int64_t words,
                           int32_t* inc_rowptr, int32_t* inc_item);

/* K10 forward: per-window mean over the N node rows.
 * Replaces: global_mean_pool(x, batch) with batch = arange(B).repeat_interleave(N)
 * (detector.py:214-215).   x : fp32 [B][N][D];  out : fp32 [B][D] */
int lg_mean_pool_fwd(const float* x, float* out, int64_t B, int64_t N, int64_t D, lg_stream_t stream);

/* K10 + NoLeakHead fused (detector.py:91-102 applied at :214-216):
 *   pooled[b] = mean_n x[b][n]                                  (global_mean_pool)
 *   hid[b]    = dropout(relu(pooled[b] W1^T + b1))              (noleak_head.mlp.0-2)
 *   logits[b*ldo + col] = hid[b] . w2 + b2                      (mlp.3, squeeze)
 * x : fp32 [B][N][D];  w1 [hidden][D], b1 [hidden], w2 [hidden], b2 [1];
 * pooled [B][D] and hid [B][hidden] are outputs saved for the backward.  hidden must
 * be 128; D in {32, 64}; dropout index b*hidden + unit.  With col = P and ldo = P+1
 * this writes the no-leak column of the (B, P+1) logits in place. */
int lg_pool_head_fwd(const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                     float* pooled, float* hid, float* logits, int64_t ldo, int64_t col,
                     int64_t B, int64_t N, int64_t D, int64_t hidden,
                     int flags, float dropout_p, uint64_t seed, uint32_t salt, lg_stream_t stream);
/* Backward: dlogits[b*ldo + col] -> dpooled fp32 [B][D] (pass to lg_pipe_scatter_bwd as
 * dpool), dw1/db1/dw2/db2 (overwritten; deterministic; db2 summed in fp64).  The ReLU /
 * dropout masks are read back from hid (> 0), scaled by 1/(1-p) under LG_F_DROPOUT. */
int64_t lg_pool_head_bwd_workspace_bytes(int64_t B, int64_t D, int64_t hidden);
int lg_pool_head_bwd(const float* pooled, const float* hid, const float* w1, const float* w2,
                     const float* dlogits, int64_t ldo, int64_t col, float* dpooled,
                     float* dw1, float* db1, float* dw2, float* db2,
                     int64_t B, int64_t D, int64_t hidden, int flags, float dropout_p,
                     void* workspace, int64_t ws_bytes, lg_stream_t stream);

/* ---------------------------------------------------------------------------
 * SharedSensorGRUEncoder (detector.py:28-73): one nn.GRU(1 [+9], H) over the
 * B*S sensor sequences (q = b*S + s), L steps, output h_L.  PyTorch gate order
 * (r, z, n) and formulas; weights in nn.GRU layout (weight_ih_l0 [3H][I],
 * weight_hh_l0 [3H][H]).  x_t = [residual[b][t][s], tfeat[b][t][0..8]] is read in
 * place — the (B*S, L, 10) concatenation of detector.py:62-67 is never built.
 *   residual : fp32 [B][L][S];  tfeat : fp32 [B][L][9] (I = 10) or NULL (I = 1)
 *   h_seq    : fp32 [L][B*S][H] every step's h (for the backward) or NULL
 *   gates    : fp32 [L][B*S][4][H] per step (r, z, n, W_hn h + b_hn) for the
 *              backward, or NULL (inference); non-NULL requires h_seq
 *   h_last   : fp32 [B*S][H]  (= h_s of detector.py:176 as [B][S][H])
 * H in {32, 64} on the tiled kernels below; any other H in 1..1024 (ABI 26; LG_EUNSUPPORTED
 * before) on the generic kernels of lg_gru_seq_fwd / lg_gru_seq_bwd in their encoder input form
 * (one hidden unit per thread, fp32 FMAs, same saved layouts: a generality path for
 * LeakDetector(sensor_hidden=...), not the bench's; the backward on min(B*S, 512) slab rows,
 * its workspace not capped by lg_gru_seq_bwd's byte budget).  I in {1, 10} (use_time
 * False/True), one layer.
 * Backward (BPTT from the saved gates, no recompute): dh_last -> dx (fp32
 * [B*S][L][I], may be NULL), dW_ih, dW_hh, db_ih, db_hh (overwritten,
 * deterministic).
 * Precision (round 4): the recurrent products of the forward and of the dx == NULL backward
 * run on the f16x2 split (two f16 parts, power-of-two scales, fp32 accumulate: |error| <=
 * 2^-22 of each product); the backward's dG scale follows a bound on the previous step's
 * maxima, so gradients of any magnitude keep that accuracy (tests/test_gpu_parity.py
 * test_gru_bwd_f16x2_scales).  The dx != NULL backward stays on fp32 MFMA. */
int lg_gru_fwd(const float* residual, const float* tfeat, const float* w_ih, const float* w_hh,
               const float* b_ih, const float* b_hh, float* h_seq, float* gates, float* h_last,
               int64_t B, int64_t L, int64_t S, int64_t I, int64_t H, lg_stream_t stream);
int64_t lg_gru_bwd_workspace_bytes(int64_t B, int64_t S, int64_t I, int64_t H);
int lg_gru_bwd(const float* residual, const float* tfeat, const float* w_ih, const float* w_hh,
               const float* h_seq, const float* gates, const float* dh_last,
               float* dx, float* dw_ih, float* dw_hh, float* db_ih, float* db_hh,
               int64_t B, int64_t L, int64_t S, int64_t I, int64_t H,
               void* workspace, int64_t ws_bytes, lg_stream_t stream);

/* Stacked GRU layers (nn.GRU(num_layers > 1); added to ABI 26 without a bump: additions only).
 * One GRU layer over a dense time-major input; layer l >= 1 of a stack reads the h_seq that
 * layer l - 1 saved (I = H, no copy), layer 0 stays lg_gru_fwd.
 *   x      : fp32 [L][Nseq][I]
 *   h_seq  : fp32 [L][Nseq][H] every step's h (required; h_L is its last step)
 *   gates  : fp32 [L][Nseq][4][H] as lg_gru_fwd, or NULL (inference)
 *   flags  : LG_F_DROPOUT: inter-layer dropout applied ON READ — the layer consumes
 *            x_eff[t][q][i] = x[t][q][i] * keep / (1 - p), keep = the counter RNG's decision for
 *            element index (t * Nseq + q) * I + i under (seed, salt) (LG_SALT_SEED_PTR honoured);
 *            x itself stays undropped (the layer below needs it for its own backward).
 * Backward: BPTT from the saved gates with dh_t += dh_seq[t] at every step.
 *   input  : dense x as above, or x == NULL and (residual, tfeat, B, S) read as lg_gru_bwd reads
 *            them (B * S == Nseq, I in {1, 10}, no dropout)
 *   dh_seq : fp32 [L][Nseq][H] or NULL;  dh_last : fp32 [Nseq][H], added at t = L - 1, or NULL
 *            (at least one of the two)
 *   dx     : dense: fp32 [L][Nseq][I], already times the same mask and scale (so it is the
 *            layer below's dh_seq as is); encoder form: [Nseq][L][I] as lg_gru_bwd; or NULL
 *   dW_ih (from x_eff), dW_hh, db_ih, db_hh: overwritten, deterministic (per-workgroup slabs,
 *   fixed-order reduction).  Workspace: lg_gru_seq_bwd_workspace_bytes (covers either input form;
 *   the generic kernel's slab rows are capped by a 256 MiB budget).
 * H in {32, 64} with dense I == H: MFMA kernels (forward on the f16x2 split, the x scale taken
 * from the data per staging chunk; backward on fp32 MFMA).  H in {32, 64} in the encoder form:
 * lg_gru_bwd's fp32 MFMA kernel.  H = 128, dense: the layers below (lg_gru_seq_tiled).  Any other
 * H, I in 1..1024: generic kernels (one hidden unit per thread).  LG_EUNSUPPORTED beyond 1024 or for other flags. */
int lg_gru_seq_fwd(const float* x, const float* w_ih, const float* w_hh, const float* b_ih,
                   const float* b_hh, float* h_seq, float* gates,
                   int64_t Nseq, int64_t L, int64_t I, int64_t H,
                   int flags, float dropout_p, uint64_t seed, uint32_t salt, lg_stream_t stream);
int64_t lg_gru_seq_bwd_workspace_bytes(int64_t Nseq, int64_t I, int64_t H);
int lg_gru_seq_bwd(const float* x, const float* residual, const float* tfeat,
                   const float* w_ih, const float* w_hh, const float* h_seq, const float* gates,
                   const float* dh_seq, const float* dh_last,
                   float* dx, float* dw_ih, float* dw_hh, float* db_ih, float* db_hh,
                   int64_t B, int64_t S, int64_t Nseq, int64_t L, int64_t I, int64_t H,
                   int flags, float dropout_p, uint64_t seed, uint32_t salt,
                   void* workspace, int64_t ws_bytes, lg_stream_t stream);

/* GRU layers at H = 128 (NormalPredictorGRU, reference models/predictor.py:84-111; added to ABI 26
 * without a bump: additions only).
 *   lg_gru_seq_tiled  1 where an MFMA kernel serves the dense form of lg_gru_seq_fwd (backward
 *                     = 0) or lg_gru_seq_bwd (backward = 1), 0 where the generic kernel does: 1
 *                     for (I, H) = (32, 32), (64, 64) and for H = 128 with any I in 1..1024.  The
 *                     dispatchers use the same predicate.
 * At H = 128 lg_gru_seq_fwd / lg_gru_seq_bwd run fp32-MFMA kernels (csrc/gru128.hip): the
 * forward keeps W_hh (and W_ih for I <= 48) in registers, a wave owning all three gates of its 16
 * units; the backward is a dh-chain recurrence that writes dG for a pass of steps into the
 * workspace, followed by GEMM launches for dW_ih, dW_hh, the bias sums and dx, their row-block
 * partials reduced in fixed order.  lg_gru_seq_bwd_workspace_bytes plans passes of up to 64 MiB
 * of dG; a larger workspace makes the passes longer.
 *   lg_gru_seq_infer  lg_gru_seq_fwd without gates, for H = 128 (LG_EUNSUPPORTED elsewhere):
 *                     h_seq [L][Nseq][H] or NULL, h_last [Nseq][H] or NULL, at least one.  With
 *                     h_seq == NULL nothing is written per step (the top layer of a stack whose
 *                     reader wants h_L alone).
 *   lg_gru_win_fwd    the shared-window form of a first layer (the residual builder, reference
 *                     models/utils.py:169-216): gi fp32 [B][T][3H] holds W_ih x + b_ih per segment
 *                     position, T >= l_pred + n_win - 1; sequence q = k * B + b (shift-major, the
 *                     reference's row order, utils.py:194-212) reads gi[b][k + t] at step t, so
 *                     the n_win windows of a segment are never unfolded.  h_seq [l_pred][n_win * B][H]
 *                     or NULL, h_last [n_win * B][H] or NULL, at least one.  H = 128
 *                     (LG_EUNSUPPORTED elsewhere).  Inference only. */
int lg_gru_seq_tiled(int64_t I, int64_t H, int backward);
int lg_gru_seq_infer(const float* x, const float* w_ih, const float* w_hh, const float* b_ih,
                     const float* b_hh, float* h_seq, float* h_last,
                     int64_t Nseq, int64_t L, int64_t I, int64_t H,
                     int flags, float dropout_p, uint64_t seed, uint32_t salt, lg_stream_t stream);
int lg_gru_win_fwd(const float* gi, const float* w_hh, const float* b_hh, float* h_seq, float* h_last,
                   int64_t B, int64_t T, int64_t l_pred, int64_t n_win, int64_t H, lg_stream_t stream);

/* The GRU encoder and the node init in one launch each way (ABI 23; the node-major trunk's
 * compressed node init, lg_node_init_bits_fwd, with the sensor projection's backward,
 * lg_sensor_proj_bwd).  Replaces detector.py:60-73 (the shared GRU) followed by :179-190 (h0,
 * the mask column, sensor_to_node, ReLU, dropout) when node_hidden == sensor_hidden == H.
 *   fwd: lg_gru_fwd's outputs, plus xs0 [S][B][H] and x0bits exactly as lg_node_init_bits_fwd
 *        writes them from h_last (W = proj_w [H][H + 1], bias = node_bias, dropout stream =
 *        (seed, salt)), except that the sensor nodes' words of x0bits are 0 (no reader:
 *        lg_gcn_fwd_nm_x0 / lg_gcn_bwd_nm_x0 take those rows from xs0).  One launch.
 *        h_seq / gates hold lg_gru_fwd's values but are PRIVATE to this pair (written here, read
 *        by lg_gru_node_init_bwd alone), in the order the kernels' lanes hold them, so that every
 *        wave store and load moves 1 KB contiguous.  Sequences come in blocks of 16, B * S rounded
 *        up: nb16 = ceil(B * S / 16), NU = H / 16,
 *          h_seq [L][nb16][NU][64][4]        gates [L][nb16][4: r, z, n, hn][NU][64][4]
 *        i.e. 16 * nb16 rows a step instead of B * S; element (t, seq, unit i) is at block
 *        seq >> 4, u = i >> 4, lane 16 * ((i >> 2) & 3) + (seq & 15), reg i & 3.  The entries of
 *        the last block's sequences >= B * S are written as 0.
 *   bwd: lg_gru_bwd without dx, its dh_last formed in the launch from the node init's
 *        pre-activation gradient, as lg_sensor_proj_bwd does: dx0 is node-major [N][B][H] (the
 *        sensor nodes' rows: lg_gcn_bwd_nm_x0 with LG_F_DX_SENSOR_ROWS), live [S] (may be NULL);
 *        also dproj_w [H][H + 1] and dproj_b [H] (+ dbias_in, the non-sensor rows' sum, which
 *        may be a pending output of an open reduce batch).  One launch + one slab reduction of
 *        all six gradients.  Workspace: lg_gru_node_init_bwd_workspace_bytes. */
int lg_gru_node_init_fwd(const float* residual, const float* tfeat, const float* w_ih, const float* w_hh,
                         const float* b_ih, const float* b_hh, float* h_seq, float* gates, float* h_last,
                         const int32_t* sensor_slot, const int64_t* sensor_idx, const float* proj_w,
                         const float* node_bias, float* xs0, uint16_t* x0bits, int64_t B, int64_t L, int64_t S,
                         int64_t I, int64_t H, int64_t N, int flags, float dropout_p, uint64_t seed, uint32_t salt,
                         lg_stream_t stream);
int64_t lg_gru_node_init_bwd_workspace_bytes(int64_t B, int64_t S, int64_t I, int64_t H);
int lg_gru_node_init_bwd(const float* residual, const float* tfeat, const float* w_ih, const float* w_hh,
                         const float* h_seq, const float* gates, const float* dx0, const int64_t* sensor_idx,
                         const float* live, const float* proj_w, const float* dbias_in, float* dw_ih, float* dw_hh,
                         float* db_ih, float* db_hh, float* dproj_w, float* dproj_b, int64_t B, int64_t L, int64_t S,
                         int64_t I, int64_t H, int64_t N, void* workspace, int64_t ws_bytes, lg_stream_t stream);

/* ---- Frozen-predictor residual builder (SURVEY 8 f rank 1) ----------------------
 * Replaces the per-window NormalPredictorTCN passes of
 * build_residual_sequence_from_segment (reference models/utils.py:169-216, TCN
 * models/predictor.py:17-81) with ONE pass per segment over the shared-window row plan
 * of models/tcn_plan.py: output row r of a conv layer reads input rows plan[r].x/.y/.z
 * (taps t, t-d, t-2d; -1 = zero padding) and, for a block's second conv, adds block-input
 * row plan[r].w (-1 = none).  Rows are segment-local; tensors are [nseg][rows][C].
 * C must be 128 (the TCN default, LG_EUNSUPPORTED otherwise); rows_out <= 2048.
 *   lg_tcn_pack_weight   Conv1d weight [C][C][3] -> packed fragment order
 *                        (lg_tcn_packed_weight_floats(C) floats), once per weight.
 *   lg_tcn_conv_fwd      y = LayerNorm(conv(x) + bias) -> ReLU (-> + residual), exact
 *                        fp32 (MFMA f32); blk = NULL for a block's first conv.  */
int64_t lg_tcn_packed_weight_floats(int64_t C);
int lg_tcn_pack_weight(const float* weight, float* packed, int64_t C, lg_stream_t stream);
int lg_tcn_conv_fwd(const float* in, const float* blk, const int32_t* plan, const float* packed_weight,
                    const float* bias, const float* ln_w, const float* ln_b, float eps, float* out,
                    int64_t nseg, int64_t rows_in, int64_t rows_blk, int64_t rows_out, int64_t C,
                    lg_stream_t stream);

/* ---- NormalPredictorTCN training: one conv stage, forward and backward ----------------
 * (Added to ABI 26 without a bump.)  The same table-driven rows as lg_tcn_conv_fwd; for
 * training a segment is one sample, row t is time step t, and the table of dilation d is
 * (t, t-d, t-2d, t or -1).  C = 128, rows_out <= 2048 and every tensor of a call below 2 GiB
 * (LG_EUNSUPPORTED otherwise; the training calls do not split into several launches).
 *   lg_tcn_conv_train_fwd  s = dropout_p(relu(LayerNorm(conv(x) + bias))), out = s + residual.
 *       Keep mask: the library's counter RNG under key(seed, salt) at element index
 *       global_row * 128 + channel, global_row over [nseg * rows_out]; LG_SALT_SEED_PTR honoured.  s (the stage output before the residual
 *       add) is always stored; out is required with blk and optional without (then out = s).
 *       xhat [nseg*rows_out][C] (normalised conv output) and rstd [nseg*rows_out] are what the
 *       backward reads; both or neither.  p = 0 without xhat / rstd is lg_tcn_conv_fwd's launch
 *       (result in out, or in s when there is no blk and s is given).
 *   lg_tcn_pack_weight_t   Conv1d weight -> packed fragment order of the backward's dx GEMM
 *       (co and ci exchanged).
 *   lg_tcn_conv_bwd        from dy (gradient of out) and the saved s, xhat, rstd:
 *       dz [nseg*rows_out][C] (gradient of the conv output), dw [C][C][3], db, dgamma, dbeta
 *       (all overwritten), and, unless dx is NULL, dx [nseg*rows_in][C] =
 *       sum_j dz[plan_t[t][j]] W_j^T + dres[plan_t[t].w]: plan_t is the transposed table
 *       (t, t+d, t+2d, row of dres or -1; -1 where no output row reads the tap), dres
 *       ([nseg][rows_res][C], may be NULL) the gradient that bypasses the stage (conv1: the
 *       block output's).  in is the stage's forward input, plan its forward table.  Row sums go
 *       through per-workgroup partials in the workspace and the fixed-order slab reduction: no
 *       atomics, equal results on every run.  ws_bytes below
 *       lg_tcn_conv_bwd_workspace_bytes(nseg, rows_out, C) is LG_EINVAL. */
int lg_tcn_pack_weight_t(const float* weight, float* packed, int64_t C, lg_stream_t stream);
int lg_tcn_conv_train_fwd(const float* in, const float* blk, const int32_t* plan, const float* packed_weight,
                          const float* bias, const float* ln_w, const float* ln_b, float eps, float p,
                          uint64_t seed, uint32_t salt, float* s, float* out, float* xhat, float* rstd,
                          int64_t nseg, int64_t rows_in, int64_t rows_blk, int64_t rows_out, int64_t C,
                          lg_stream_t stream);
int64_t lg_tcn_conv_bwd_workspace_bytes(int64_t nseg, int64_t rows_out, int64_t C);
int lg_tcn_conv_bwd(const float* dy, const float* s, const float* xhat, const float* rstd, const float* in,
                    const float* dres, const int32_t* plan, const int32_t* plan_t, const float* packed_weight_t,
                    const float* ln_w, float p, float* dz, float* dx, float* dw, float* db, float* dgamma,
                    float* dbeta, int64_t nseg, int64_t rows_in, int64_t rows_res, int64_t rows_out, int64_t C,
                    void* workspace, int64_t ws_bytes, lg_stream_t stream);

/* ---- Predictor training tail: head = nn.Linear(H, S) on h_last, then nn.MSELoss() ------
 * (reference models/train_predictor.py: loss_fn(model(x, x_time), y); added to ABI 26 without a
 * bump: additions only.)  All tensors fp32 and contiguous: h [B][H], weight [S][H], bias [S],
 * target [B][S].
 *   fwd: y_hat [B][S] = h weight^T + bias (saved for the backward), loss (device scalar) =
 *        mean((y_hat - target)^2) over B * S elements, ONE launch: rowsq [B] scratch takes each
 *        row's sum of squares, and the workgroup that finishes last sums the rows in row order
 *        (fp64).  counter: as for the cross-entropy forward above (a device uint32, 0 between
 *        launches, one per stream).  weight is staged in LDS when S * H <= 39,936 floats and its
 *        address is 16-byte aligned, else read through L2.
 *   bwd: with d = 2 grad_loss[0] / (B S) (y_hat - target): dh [B][H] = d weight, dweight [S][H]
 *        = d^T h, dbias [S] = sum_b d.  One kernel launch writes dh and per-chunk partials of
 *        [dweight | dbias] into the workspace; the fixed-order slab reduction (fp64, inside a
 *        reduce batch when one is open) forms dweight and dbias.  No float atomics: equal bits on
 *        every run.  Every output is overwritten.  ws_bytes below the workspace size is LG_EINVAL.
 * Range: B >= 1, 1 <= H <= 1024, 1 <= S <= 1024, B * max(H, S) * 4 < 2^31; outside it, or with a
 * null pointer, LG_EINVAL before any HIP call.  Tested against an fp64 CPU formula in
 * tests/test_gpu_head_mse.py. */
int lg_head_mse_fwd(const float* h, const float* weight, const float* bias, const float* target, int64_t B,
                    int64_t H, int64_t S, float* y_hat, float* rowsq, float* loss, unsigned* counter,
                    lg_stream_t stream);
int64_t lg_head_mse_bwd_workspace_bytes(int64_t B, int64_t H, int64_t S);
int lg_head_mse_bwd(const float* h, const float* weight, const float* target, const float* y_hat,
                    const float* grad_loss, int64_t B, int64_t H, int64_t S, float* dh, float* dweight,
                    float* dbias, void* workspace, int64_t ws_bytes, lg_stream_t stream);

/* ---- Device sampler: the datasets' per-sample draws and the window gather --------------
 * (models/datasets.py AbruptLeakDetectorDataset.draw / NormalPredictorDataset.draw, reference
 * datasets.py:236-243, 483-517; added to ABI 26 without a bump: additions only.)
 * Sample idx of a dataset is a pure function of numpy's default_rng(seed + idx).  The draw entry
 * points replay that stream (csrc/np_rng.h: SeedSequence, PCG64, random(), integers(), scalar
 * choice()) for the n samples idx = i0 .. i0 + n - 1, one thread per sample, and write one
 * int32[LG_DRAW_RECORD] record per sample:
 *   [bank scene index, t, label, pipe_index, bucket code, attempts, 0, 0]
 * (bucket codes: 0 early, 1 late, 2 pre, 3 noleak; -1 for the predictor).  seed + idx is taken
 * modulo 2^64: callers keep it below 2^64, where numpy's entropy has at most two 32-bit words.
 *   lg_draw_detector   tables over the n_scenes scenes of the HBM bank: leak_list [n_leak] and
 *       noleak_list [n_noleak] hold the bank index of each entry of the dataset's two scene lists
 *       (choice draws a POSITION in the list); times [n_scenes][4][2] is (start, count) of the
 *       scene's time list per bucket (every list is a contiguous arange; count 0 = empty, the
 *       attempt is repeated, up to 10); pipe [n_scenes] the scene's pipe index (-1: no-leak scene).
 *       cum_host: the four cumulative bucket probabilities (fp64, compared as the dataset compares
 *       them).  label = pipe for early / late, no_leak_class for pre / noleak.
 *   lg_draw_predictor  scene = scene_list[choice(n_list)], t = integers(l_in - 1, scene_len[scene] - h).
 * A sample that cannot be decided (ten empty time lists; a list entry outside [0, n_scenes); a
 * scene shorter than l_in + h) gets the record [-1, -1, -1, -1, -1, attempts, 0, 0] and adds 1 to
 * err[0]; nothing else happens on the device.  err is TWO device uint32 words, zeroed by the caller.
 * n <= LG_DRAW_MAX_SAMPLES per call; a null pointer or a size out of range is LG_EINVAL before any
 * HIP call.  Populations of 2^32 entries or more are refused with LG_EINVAL, never truncated.
 *   lg_gather_windows  one workgroup per sample s of records[0 .. n): up to three segments k (src_k
 *       NULL = unused), dst_k[s] = src_k[scene][t + off_k .. t + off_k + len_k) as len_k * C_k
 *       floats (src_k is a bank tensor [n_scenes][T_max][C_k], dst_k [n][len_k][C_k]; dword
 *       copies, rows are only 4-byte aligned), plus label / pipe_index (int64) and bucket_code
 *       (int32) of the sample (each may be NULL).  A record with label < 0 yields zeros and -1s and
 *       no address is formed from it; a record whose windows do not lie inside the bank is treated
 *       the same and adds 1 to err[1].
 *   *_host             the same draw code on the CPU over host tables (tests, no device needed).
 *   lg_np_stream_host  replays a script of n calls on default_rng(seed): ops_host[k] LG_NP_RANDOM ->
 *       out_f_host[k] = random(); LG_NP_BOUNDED -> out_i_host[k] = integers(low_host[k],
 *       low_host[k] + count_host[k]), 1 <= count <= 2^32 (else LG_EINVAL, before any draw). */
#define LG_DRAW_RECORD 8
#define LG_DRAW_MAX_SAMPLES (1 << 20)
#define LG_NP_RANDOM 0
#define LG_NP_BOUNDED 1
int lg_draw_detector(uint64_t seed, int64_t i0, int64_t n, const int32_t* leak_list, int64_t n_leak,
                     const int32_t* noleak_list, int64_t n_noleak, const int32_t* times, const int32_t* pipe,
                     int64_t n_scenes, const double* cum_host, int64_t no_leak_class, int32_t* records,
                     uint32_t* err, lg_stream_t stream);
int lg_draw_detector_host(uint64_t seed, int64_t i0, int64_t n, const int32_t* leak_list_host, int64_t n_leak,
                          const int32_t* noleak_list_host, int64_t n_noleak, const int32_t* times_host,
                          const int32_t* pipe_host, int64_t n_scenes, const double* cum_host,
                          int64_t no_leak_class, int32_t* records_host, uint32_t* err_host);
int lg_draw_predictor(uint64_t seed, int64_t i0, int64_t n, const int32_t* scene_list, int64_t n_list,
                      const int32_t* scene_len, int64_t n_scenes, int64_t l_in, int64_t h, int32_t* records,
                      uint32_t* err, lg_stream_t stream);
int lg_draw_predictor_host(uint64_t seed, int64_t i0, int64_t n, const int32_t* scene_list_host, int64_t n_list,
                           const int32_t* scene_len_host, int64_t n_scenes, int64_t l_in, int64_t h,
                           int32_t* records_host, uint32_t* err_host);
int lg_np_stream_host(uint64_t seed, const int32_t* ops_host, const int64_t* low_host, const uint64_t* count_host,
                      int64_t n, double* out_f_host, int64_t* out_i_host);
int lg_gather_windows(const int32_t* records, int64_t n, int64_t n_scenes, int64_t T_max,
                      const float* src0, int64_t C0, int64_t off0, int64_t len0, float* dst0,
                      const float* src1, int64_t C1, int64_t off1, int64_t len1, float* dst1,
                      const float* src2, int64_t C2, int64_t off2, int64_t len2, float* dst2,
                      int64_t* label, int64_t* pipe_index, int32_t* bucket_code, uint32_t* err,
                      lg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* LEAKGNN_H */
