// Evaluator tails: what turns the detector's (B, P+1) logits into decisions and counts.
//   lg_window_metrics : DetectorEvaluator.evaluate's per-batch tail (reference
//                       window_evaluator.py:227-483; torch: argmax, topk, a full argsort, scatter,
//                       gather, two mask indexings and ~40 mask sums) as ONE launch;
//   lg_event_decide   : the event evaluator's trigger and aggregation (reference
//                       event_evaluator.py:327-342) as TWO launches, nothing read back in between.
// Both are row scans over C = P+1 floats, one wave per row, the shape of k_ce_fwd (loss.hip).
//
// One total order on a row's entries decides everything (include/leakgnn.h): a precedes b when a's
// value is greater (NaN above +inf, -0 == +0), or the values are equal and a's index is lower.
// wm_key folds it into one 64-bit integer, greater = earlier: the value as a monotone 32-bit code in
// the high word, 2^32 - 1 - index in the low word.  A row's best entry is then an integer max and
// the position of an entry is a count of greater keys, so no sort is needed, every tie has a defined
// answer, and a row is read ONCE: the keys of logits[row, label] and logits[row, min(label, nlc-1)]
// are fetched before the stream starts.
//
// Counters are integers end to end: a row's outcome is a bit mask over the counter slots (the same
// in every lane), lane l of the wave keeps slot l's count in a register across the wave's rows, the
// workgroup adds its waves through LDS and issues one 64-bit integer vector atomic per nonzero slot.
// No float atomics: the result does not depend on scheduling.
#include <algorithm>
#include <climits>
#include "common.h"

namespace {

constexpr int kWmWaves = 4;
constexpr int kWmThreads = 64 * kWmWaves;
constexpr int kWmUnroll = 8;  // row elements per lane in flight (C = 765: two rounds)
constexpr int kEvThreads = 1024;
constexpr uint64_t kWmNoKey = ~uint64_t{0};  // no entry's key is greater: its counts stay 0

// slot layout of `counters` (LG_WM_COUNTERS slots; models/ops.py WINDOW_COUNTERS is its mirror)
enum : int {
    kTotal = 0, kCorrect1, kCorrectK, kNlTotal, kNlCorrect, kLeakTotal, kLeakCorrect1, kLeakCorrectK,
    kTp, kFp, kFn, kTn,
    kBucket0,                          // 4 buckets x (b_total, b_correct1, b_correctk, b_pred_nl)
    kPreFalseAlarm = kBucket0 + 16, kNoleakFalseAlarm,
    kSuccess0,                         // LG_WM_MAX_LIST radii
    kAccI0 = kSuccess0 + LG_WM_MAX_LIST,
    kBadLabel = kAccI0 + LG_WM_MAX_LIST,
    kWmSlots
};
static_assert(kWmSlots == LG_WM_COUNTERS, "counter layout");
static_assert(kWmSlots <= 64, "one lane per counter slot");

__device__ __forceinline__ uint64_t wm_key(float v, uint32_t idx) {
    const uint32_t u = __float_as_uint(v);
    uint32_t k;
    if (v != v) k = 0xFFFFFFFFu;             // NaN: above +inf (torch's argmax rule)
    else if (v == 0.f) k = 0x80000000u;      // -0 and +0 are one value
    else k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return (static_cast<uint64_t>(k) << 32) | (0xFFFFFFFFu - idx);
}
__device__ __forceinline__ uint32_t wm_key_index(uint64_t key) { return 0xFFFFFFFFu - static_cast<uint32_t>(key); }

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t hi = __shfl_xor(static_cast<uint32_t>(v >> 32), o);
        const uint32_t lo = __shfl_xor(static_cast<uint32_t>(v), o);
        const uint64_t other = (static_cast<uint64_t>(hi) << 32) | lo;
        v = other > v ? other : v;
    }
    return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

struct WmScan {
    uint64_t best;  // key of the row's first entry
    int before_a;   // entries of the row that precede key a
    int before_b;   // entries with index < nb that precede key b
};

// One pass over a row by one wave, coalesced (lane l reads columns l + 64 k); every lane returns
// the wave's result.  The one place the order is applied to a row: both evaluators call it.
__device__ __forceinline__ WmScan wm_scan(const float* __restrict__ row, int64_t C, uint64_t ka, uint64_t kb,
                                          int64_t nb, int lane) {
    uint64_t best = 0;  // below every entry's key (an entry's value code is never 0)
    int na = 0, nbf = 0;
    for (int64_t c0 = 0; c0 < C; c0 += 64 * kWmUnroll) {
        float v[kWmUnroll];
#pragma unroll
        for (int k = 0; k < kWmUnroll; ++k) {
            const int64_t c = c0 + lane + 64 * k;
            v[k] = c < C ? row[c] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < kWmUnroll; ++k) {
            const int64_t c = c0 + lane + 64 * k;
            if (c < C) {
                const uint64_t key = wm_key(v[k], static_cast<uint32_t>(c));
                best = key > best ? key : best;
                na += key > ka ? 1 : 0;
                nbf += (c < nb && key > kb) ? 1 : 0;
            }
        }
    }
    return WmScan{wave_max_u64(best), wave_sum_i32(na), wave_sum_i32(nbf)};
}

struct WmArgs {
    const float* x;
    const int64_t* label;
    int64_t B, C, ldx, nlc, topk;
    const int32_t* bucket;
    const double* dist;
    const int32_t* inv_rank;
    int R, I;
    double radii[LG_WM_MAX_LIST];
    int64_t acc_is[LG_WM_MAX_LIST];
    unsigned long long* counters;
    int32_t* rank_out;
    double* atd_out;
};

__global__ void __launch_bounds__(kWmThreads) k_window_metrics(WmArgs a) {
    __shared__ unsigned s_cnt[kWmWaves][64];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;  // w: scalar
    unsigned cnt = 0;  // lane l: how many of this wave's rows raised counter slot l
    for (int64_t b = static_cast<int64_t>(blockIdx.x) * kWmWaves + w; b < a.B;
         b += static_cast<int64_t>(gridDim.x) * kWmWaves) {
        const int64_t lab = a.label[b];  // everything below is the same in every lane
        uint64_t mask = 0;
        int32_t rank = 0;
        double atd = __builtin_nan("");
        if (lab < 0 || lab >= a.C) {
            mask = uint64_t{1} << kBadLabel;  // counted here and nowhere else; nothing read at `lab`
        } else {
            const float* row = a.x + b * a.ldx;
            const int64_t lp = lab < a.nlc ? lab : a.nlc - 1;
            const uint64_t klab = wm_key(row[lab], static_cast<uint32_t>(lab));
            const uint64_t kpipe = wm_key(row[lp], static_cast<uint32_t>(lp));
            const WmScan s = wm_scan(row, a.C, klab, kpipe, a.nlc, lane);
            const int64_t pred1 = wm_key_index(s.best);
            const bool hit1 = pred1 == lab;
            const bool hitk = s.before_a < (a.topk < a.C ? a.topk : a.C);
            const bool is_nl = lab == a.nlc, is_leak = !is_nl;
            const bool pred_nl = pred1 == a.nlc, pred_leak = !pred_nl;
            auto bit = [&](int slot, bool on) { mask |= static_cast<uint64_t>(on) << slot; };
            bit(kTotal, true);
            bit(kCorrect1, hit1);
            bit(kCorrectK, hitk);
            bit(kNlTotal, is_nl);
            bit(kNlCorrect, hit1 && is_nl);
            bit(kLeakTotal, is_leak);
            bit(kLeakCorrect1, hit1 && is_leak);
            bit(kLeakCorrectK, hitk && is_leak);
            bit(kTp, pred_leak && is_leak);
            bit(kFp, pred_leak && is_nl);
            bit(kFn, pred_nl && is_leak);
            bit(kTn, pred_nl && is_nl);
            if (a.bucket) {
                const int32_t bc = a.bucket[b];
                if (bc >= 0 && bc < 4) {
                    bit(kBucket0 + 4 * bc + 0, true);
                    bit(kBucket0 + 4 * bc + 1, hit1);
                    bit(kBucket0 + 4 * bc + 2, hitk);
                    bit(kBucket0 + 4 * bc + 3, pred_nl);
                }
                bit(kPreFalseAlarm, is_nl && pred_leak && bc == 2);
                bit(kNoleakFalseAlarm, is_nl && pred_leak && bc == 3);
            }
            if (is_leak) {
                rank = 1 + s.before_b;
                if (a.dist) {
                    // the tables are (nlc, nlc): a missed row, or a leak label past nlc (C > nlc + 1),
                    // looks nothing up; a prediction past nlc is clamped, as the torch route clamps it
                    const bool look = pred_leak && lab < a.nlc;
                    const int64_t pc = pred1 < a.nlc ? pred1 : a.nlc - 1;
                    atd = look ? a.dist[lab * a.nlc + pc] : __builtin_huge_val();
#pragma unroll
                    for (int r = 0; r < LG_WM_MAX_LIST; ++r) bit(kSuccess0 + r, r < a.R && atd <= a.radii[r]);
                    if (a.inv_rank && look) {
                        const int64_t pos = a.inv_rank[pc * a.nlc + lab];
#pragma unroll
                        for (int i = 0; i < LG_WM_MAX_LIST; ++i)
                            bit(kAccI0 + i, i < a.I && pos < a.acc_is[i] && a.acc_is[i] > 0);
                    }
                }
            }
        }
        if (lane == 0) {
            a.rank_out[b] = rank;
            if (a.atd_out) a.atd_out[b] = atd;
        }
        cnt += static_cast<unsigned>((mask >> lane) & 1u);
    }
    s_cnt[w][lane] = cnt;
    __syncthreads();
    if (w == 0 && lane < kWmSlots) {
        unsigned tot = 0;
#pragma unroll
        for (int i = 0; i < kWmWaves; ++i) tot += s_cnt[i][lane];
        if (tot) atomicAdd(a.counters + lane, static_cast<unsigned long long>(tot));
    }
}

// ---------------------------------------------------------------------------------------------
// Event decision.  Launch 1: alarm[i] = [first entry of row i != noleak], one wave per row.
// Launch 2, ONE workgroup: trig = first alarm, stop = first i >= trig whose end time is agg_ns or
// more after trig's (at least trig + 1, W when there is none), then one thread per column adds rows
// trig .. stop - 1 in row order in plain fp32 (the bits of event_evaluator.sum_logits_from) and the
// workgroup takes the first entry of that sum.
__global__ void __launch_bounds__(kWmThreads)
k_event_alarm(const float* __restrict__ x, int64_t W, int64_t C, int64_t ldx, int64_t noleak,
              int32_t* __restrict__ alarm) {
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    for (int64_t r = static_cast<int64_t>(blockIdx.x) * kWmWaves + w; r < W;
         r += static_cast<int64_t>(gridDim.x) * kWmWaves) {
        const WmScan s = wm_scan(x + r * ldx, C, kWmNoKey, kWmNoKey, 0, lane);
        if (lane == 0) alarm[r] = static_cast<int64_t>(wm_key_index(s.best)) != noleak ? 1 : 0;
    }
}

// max over the workgroup, returned to every thread; `sm` (one slot per wave) is free again on return
__device__ __forceinline__ uint64_t block_max_u64(uint64_t v, uint64_t* sm) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    v = wave_max_u64(v);
    if (lane == 0) sm[w] = v;
    __syncthreads();
    uint64_t m = 0;
    for (int i = 0; i < kEvThreads / 64; ++i) m = sm[i] > m ? sm[i] : m;
    __syncthreads();
    return m;
}
// first index (min) as a max: indices are in [0, W], W <= INT64_MAX
__device__ __forceinline__ int64_t block_min_index(int64_t v, uint64_t* sm) {
    return static_cast<int64_t>(~block_max_u64(~static_cast<uint64_t>(v), sm));
}

__global__ void __launch_bounds__(kEvThreads)
k_event_decide(const float* __restrict__ x, const int64_t* __restrict__ end_ns, const int32_t* __restrict__ alarm,
               int64_t W, int64_t C, int64_t ldx, int64_t agg_ns, int64_t* __restrict__ out,
               float* __restrict__ summed) {
    __shared__ uint64_t sm[kEvThreads / 64];
    const int tid = threadIdx.x;
    int64_t t = W;
    for (int64_t i = tid; i < W; i += kEvThreads)
        if (alarm[i]) {
            t = i;
            break;
        }
    const int64_t trig = block_min_index(t, sm);
    if (trig >= W) {  // no alarm (the same in every thread)
        if (tid < 3) out[tid] = -1;
        if (summed)
            for (int64_t c = tid; c < C; c += kEvThreads) summed[c] = 0.f;
        return;
    }
    const int64_t t0 = end_ns[trig];
    int64_t st = W;
    for (int64_t i = trig + tid; i < W; i += kEvThreads)
        if (end_ns[i] - t0 >= agg_ns) {
            st = i;
            break;
        }
    int64_t stop = block_min_index(st, sm);
    stop = stop > trig ? stop : trig + 1;
    uint64_t best = 0;
    for (int64_t c = tid; c < C; c += kEvThreads) {
        const float* col = x + c;
        float s = col[trig * ldx];
#pragma unroll 8
        for (int64_t i = trig + 1; i < stop; ++i) s = s + col[i * ldx];
        if (summed) summed[c] = s;
        const uint64_t key = wm_key(s, static_cast<uint32_t>(c));
        best = key > best ? key : best;
    }
    best = block_max_u64(best, sm);
    if (tid == 0) {
        out[0] = trig;
        out[1] = stop;
        out[2] = wm_key_index(best);
    }
}

}  // namespace

extern "C" int lg_window_metrics(const float* logits, const int64_t* label, int64_t B, int64_t C, int64_t ldx,
                                 int64_t nlc, int64_t topk, const int32_t* bucket, const double* dist,
                                 const int32_t* inv_rank, const double* radii_host, int R, const int64_t* acc_is_host,
                                 int I, int64_t* counters, int64_t n_counters, int32_t* rank_out, double* atd_out,
                                 lg_stream_t stream) {
    if (B < 0 || C < 2 || ldx < C || nlc < 1 || nlc > C - 1 || topk < 1) return LG_EINVAL;
    if (R < 0 || R > LG_WM_MAX_LIST || I < 0 || I > LG_WM_MAX_LIST) return LG_EINVAL;
    if ((R > 0 && !radii_host) || (I > 0 && !acc_is_host)) return LG_EINVAL;
    if (inv_rank && !dist) return LG_EINVAL;
    if (!counters || n_counters != LG_WM_COUNTERS) return LG_EINVAL;
    if (B == 0) return LG_OK;
    if (!logits || !label || !rank_out || (dist && !atd_out)) return LG_EINVAL;
    if (C > INT32_MAX) return LG_EUNSUPPORTED;  // 32-bit column indices in the keys
    WmArgs a{};
    a.x = logits;
    a.label = label;
    a.B = B, a.C = C, a.ldx = ldx, a.nlc = nlc, a.topk = topk;
    a.bucket = bucket;
    a.dist = dist;
    a.inv_rank = inv_rank;
    a.R = R, a.I = I;
    for (int r = 0; r < R; ++r) a.radii[r] = radii_host[r];
    for (int i = 0; i < I; ++i) a.acc_is[i] = acc_is_host[i];
    a.counters = reinterpret_cast<unsigned long long*>(counters);
    a.rank_out = rank_out;
    a.atd_out = dist ? atd_out : nullptr;
    const int grid = static_cast<int>(std::min<int64_t>((B + kWmWaves - 1) / kWmWaves, 4 * lg_num_cus()));
    lg_launch(k_window_metrics, grid, kWmThreads, 0, lg_stream(stream), a);
    LG_RET_IF_LAUNCH_FAILED();
    return LG_OK;
}

extern "C" int64_t lg_event_decide_workspace_bytes(int64_t W) { return W > 0 ? 4 * W : 0; }

extern "C" int lg_event_decide(const float* logits, const int64_t* end_ns, int64_t W, int64_t C, int64_t ldx,
                               int64_t agg_ns, int64_t noleak, int64_t* out, float* summed, void* workspace,
                               int64_t workspace_bytes, lg_stream_t stream) {
    if (W < 0 || C < 1 || ldx < C || noleak < 0 || noleak >= C || !out) return LG_EINVAL;
    if (W > 0 && (!logits || !end_ns || !workspace || workspace_bytes < lg_event_decide_workspace_bytes(W)))
        return LG_EINVAL;
    if (C > INT32_MAX) return LG_EUNSUPPORTED;
    hipStream_t s = lg_stream(stream);
    int32_t* alarm = static_cast<int32_t*>(workspace);
    if (W > 0) {
        const int grid = static_cast<int>(std::min<int64_t>((W + kWmWaves - 1) / kWmWaves, 8 * lg_num_cus()));
        lg_launch(k_event_alarm, grid, kWmThreads, 0, s, logits, W, C, ldx, noleak, alarm);
        LG_RET_IF_LAUNCH_FAILED();
    }
    lg_launch(k_event_decide, 1, kEvThreads, 0, s, logits, end_ns, alarm, W, C, ldx, agg_ns, out, summed);
    LG_RET_IF_LAUNCH_FAILED();
    return LG_OK;
}
