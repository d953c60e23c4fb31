// The training loss (reference train_detector.py:235, 311: nn.CrossEntropyLoss(), mean
// reduction, ignore_index -100) over the (B, P+1) logits, forward and backward.  torch runs
// it as six launches (log_softmax, nll forward, two fills, nll backward, log_softmax
// backward); here:
//   forward : one wave per row: lse = max + log(sum exp(x - max)) (fp32, fixed lane order
//             then a fixed shuffle tree), row loss = lse - x[target] -> lse[b], rowloss[b];
//             the workgroup that finishes last sums the counted rows in row order
//             (deterministic), in the same launch.  The hand-off is fence-free
//             (MI355X_MICROARCH.md, the sc1 hand-off table's first row): the row losses are
//             stored sc1 (agent-scope relaxed atomic stores, 4 B), every wave waits for its
//             stores (vmcnt 0), then behind a workgroup barrier one lane adds to the counter
//             (agent scope); the workgroup whose add returns gridDim - 1 reads the row losses
//             with sc1 loads and resets the counter.  (Round 3 took the mean behind a release /
//             acquire fence pair: on gfx950 that is an L2 writeback + invalidate in every
//             workgroup — buffer_wbl2 / buffer_inv — which, right after the EdgeHead forward's
//             100 MB of stores, made the launch 12 us for 0.8 MB of logits; round 4 ran the
//             mean as a second, single-wave launch, ~5 us in the step.)
//   backward: dx[b][c] = g / n * (exp(x - lse[b]) - [c == target[b]])   (0 for ignored rows)
// lse[b] is one float, so it rounds at the size of the logits: by at most 2^-20 = 9.5e-7 below
// kCeLseFine = 32 (the absolute error it leaves in lse - x[target] and the relative error in
// exp(x - lse): under 1e-6), by 4.9e-4 at logits near 1e4, where it was 50 x the loss's
// bar (tests/test_gpu_step_tail.py).  Rows whose |lse| is not below kCeLseFine therefore take
// the row loss as (max - x[target]) + log(sum) and the softmax as exp(x - max) / sum, the
// backward finding the row's max and sum again; all other rows keep the one-pass forms above.
#include <algorithm>
#include "common.h"

namespace {

constexpr int kCeWaves = 4;
constexpr int kCeThreads = 64 * kCeWaves;
constexpr int kCePer = 16;  // row elements per lane held in registers (C <= 1024)
constexpr float kCeLseFine = 32.f;  // below it lse[b]'s rounding is under 1e-6 (header)

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the mean over the counted rows, in row order (one wave; sc1 loads: the rows were stored sc1
// by other workgroups of the same launch)
__device__ __forceinline__ void ce_mean_wave(float* rowloss, const int64_t* __restrict__ target, int64_t B,
                                             int64_t ignore, float* __restrict__ loss) {
    const int lane = threadIdx.x & 63;
    float acc = 0.f, cnt = 0.f;
    for (int64_t b0 = 0; b0 < B; b0 += 64) {
        const int64_t b = b0 + lane;
        float v = 0.f, c = 0.f;
        if (b < B) {
            v = __hip_atomic_load(rowloss + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            c = target[b] == ignore ? 0.f : 1.f;
        }
        acc += wave_sum(v);
        cnt += wave_sum(c);
    }
    if (lane == 0) loss[0] = acc / cnt;  // NaN when every row is ignored, as torch
}

__global__ void __launch_bounds__(kCeThreads)
k_ce_fwd(const float* __restrict__ x, const int64_t* __restrict__ target, int64_t B, int64_t C, int64_t ldx,
         int64_t ignore, float* __restrict__ lse, float* rowloss, unsigned* counter, float* __restrict__ loss) {
    __shared__ unsigned is_last;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t b = static_cast<int64_t>(blockIdx.x) * kCeWaves + w; b < B; b += static_cast<int64_t>(gridDim.x) * kCeWaves) {
        const float* row = x + b * ldx;
        float m = -__builtin_huge_valf(), s = 0.f;
        if (C <= 64 * kCePer) {  // the whole row in registers: every load in flight at once
            float v[kCePer];
#pragma unroll
            for (int k = 0; k < kCePer; ++k) {
                const int64_t c = lane + 64 * k;
                v[k] = c < C ? row[c] : -__builtin_huge_valf();
            }
#pragma unroll
            for (int k = 0; k < kCePer; ++k) m = fmaxf(m, v[k]);
            m = wave_max(m);
#pragma unroll
            for (int k = 0; k < kCePer; ++k) s += lane + 64 * k < C ? expf(v[k] - m) : 0.f;
        } else {
            for (int64_t c = lane; c < C; c += 64) m = fmaxf(m, row[c]);
            m = wave_max(m);
            for (int64_t c = lane; c < C; c += 64) s += expf(row[c] - m);
        }
        s = wave_sum(s);
        const float ls = logf(s);
        const float l = m + ls;
        if (lane == 0) {
            const int64_t t = target[b];
            lse[b] = l;
            // a target outside [0, C) (torch raises) poisons the loss with NaN, never reads out of bounds
            float rl = t == ignore ? 0.f : __builtin_nanf("");
            if (t >= 0 && t < C && t != ignore) rl = fabsf(l) < kCeLseFine ? l - row[t] : (m - row[t]) + ls;
            __hip_atomic_store(rowloss + b, rl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's row losses have left
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned old = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        is_last = old + 1 == gridDim.x ? 1u : 0u;
    }
    __syncthreads();
    if (!is_last) return;
    if (w == 0) ce_mean_wave(rowloss, target, B, ignore, loss);
    if (threadIdx.x == 0) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(kCeThreads)
k_ce_bwd(const float* __restrict__ x, const int64_t* __restrict__ target, const float* __restrict__ lse,
         const float* __restrict__ gout, int64_t B, int64_t C, int64_t ldx, int64_t ignore, float* __restrict__ dx,
         int64_t ldd) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // n = counted rows (every workgroup counts them the same way)
    float cnt = 0.f;
    for (int64_t b0 = 0; b0 < B; b0 += 64) {
        const int64_t b = b0 + lane;
        cnt += wave_sum((b < B && target[b] != ignore) ? 1.f : 0.f);
    }
    const float g = gout[0] / cnt;
    for (int64_t b = static_cast<int64_t>(blockIdx.x) * kCeWaves + w; b < B; b += static_cast<int64_t>(gridDim.x) * kCeWaves) {
        const float* row = x + b * ldx;
        float* drow = dx + b * ldd;
        const int64_t t = target[b];
        const float l = lse[b];
        const float gi = t == ignore ? 0.f : g;
        const bool fine = fabsf(l) < kCeLseFine;  // the same in every lane
        if (C <= 64 * kCePer) {
            float v[kCePer];
#pragma unroll
            for (int k = 0; k < kCePer; ++k) {
                const int64_t c = lane + 64 * k;
                v[k] = c < C ? row[c] : 0.f;
            }
            if (fine) {
#pragma unroll
                for (int k = 0; k < kCePer; ++k) {
                    const int64_t c = lane + 64 * k;
                    if (c < C) drow[c] = gi * (expf(v[k] - l) - (c == t ? 1.f : 0.f));
                }
            } else {
                float m = -__builtin_huge_valf(), s = 0.f;
#pragma unroll
                for (int k = 0; k < kCePer; ++k) m = lane + 64 * k < C ? fmaxf(m, v[k]) : m;
                m = wave_max(m);
#pragma unroll
                for (int k = 0; k < kCePer; ++k) {
                    v[k] = lane + 64 * k < C ? expf(v[k] - m) : 0.f;
                    s += v[k];
                }
                const float rs = 1.f / wave_sum(s);
#pragma unroll
                for (int k = 0; k < kCePer; ++k) {
                    const int64_t c = lane + 64 * k;
                    if (c < C) drow[c] = gi * (v[k] * rs - (c == t ? 1.f : 0.f));
                }
            }
        } else if (fine) {
            for (int64_t c = lane; c < C; c += 64) drow[c] = gi * (expf(row[c] - l) - (c == t ? 1.f : 0.f));
        } else {
            float m = -__builtin_huge_valf(), s = 0.f;
            for (int64_t c = lane; c < C; c += 64) m = fmaxf(m, row[c]);
            m = wave_max(m);
            for (int64_t c = lane; c < C; c += 64) s += expf(row[c] - m);
            const float rs = 1.f / wave_sum(s);
            for (int64_t c = lane; c < C; c += 64) drow[c] = gi * (expf(row[c] - m) * rs - (c == t ? 1.f : 0.f));
        }
    }
}

}  // namespace

extern "C" int lg_cross_entropy_fwd(const float* logits, const int64_t* target, int64_t B, int64_t C, int64_t ldx,
                                    int64_t ignore_index, float* loss, float* lse, float* rowloss, unsigned* counter,
                                    lg_stream_t stream) {
    if (B < 0 || C <= 0 || ldx < C || !loss || !counter) return LG_EINVAL;
    hipStream_t s = lg_stream(stream);
    if (B == 0) {  // the mean over no rows is NaN (torch); a memset node, so the call stays capturable
        return hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(loss), 0x7FC00000, 1, s) == hipSuccess ? LG_OK
                                                                                                          : LG_EHIP;
    }
    if (!logits || !target || !lse || !rowloss) return LG_EINVAL;
    // at most one workgroup per CU: every workgroup of the launch is co-resident, so the last
    // ticket is taken only after every workgroup's row losses have left (the fence-free
    // hand-off above was validated at this grid; larger B loops inside the workgroups,
    // tests/test_gpu_library.py::test_cross_entropy_matches_torch at B = 65,536)
    const int grid = static_cast<int>(std::min<int64_t>((B + kCeWaves - 1) / kCeWaves, lg_num_cus()));
    lg_launch(k_ce_fwd, grid, kCeThreads, 0, s, logits, target, B, C, ldx, ignore_index, lse, rowloss, counter, loss);
    LG_RET_IF_LAUNCH_FAILED();
    return LG_OK;
}

extern "C" int lg_cross_entropy_bwd(const float* logits, const int64_t* target, const float* lse,
                                    const float* grad_loss, int64_t B, int64_t C, int64_t ldx, int64_t ignore_index,
                                    float* dlogits, int64_t ldd, lg_stream_t stream) {
    if (B < 0 || C <= 0 || ldx < C || ldd < C || !grad_loss) return LG_EINVAL;
    if (B == 0) return LG_OK;
    if (!logits || !target || !lse || !dlogits) return LG_EINVAL;
    hipStream_t s = lg_stream(stream);
    const int grid = static_cast<int>(std::min<int64_t>((B + kCeWaves - 1) / kCeWaves, 4 * lg_num_cus()));
    lg_launch(k_ce_bwd, grid, kCeThreads, 0, s, logits, target, lse, grad_loss, B, C, ldx, ignore_index, dlogits, ldd);
    LG_RET_IF_LAUNCH_FAILED();
    return LG_OK;
}

// ---------------------------------------------------------------------------------------------
// The same loss with class weights w[C], label smoothing eps over a table U[C][C] (absent: the
// uniform 1/C, torch's label_smoothing) and the three reductions (include/leakgnn.h,
// lg_cross_entropy_opt_fwd): for a counted row b (target y != ignore_index, 0 <= y < C)
//   a[c] = w[c] * ((1 - eps) * [c == y] + eps * U[y][c])      S = sum_c a[c]
//   row  = S * lse - sum_c a[c] * x[c]                         dx[c] = G * (S * softmax[c] - a[c])
// One wave per row and the lane mapping of k_ce_fwd: lane `lane` holds columns lane + 64 k of the
// logits, of w and of U's row y, so a[c] is formed in registers and needs no LDS.  The row loss is
// summed as sum_c a[c] * (lse - x[c]) (|lse| < kCeLseFine) or S * log(sum) + sum_c a[c] * (max - x[c]),
// the two-form rule above; a term with a[c] == 0 is skipped, so it is exactly 0 where x[c] = -inf.
// mean / sum: the hand-off of k_ce_fwd, unchanged (sc1 row losses, vmcnt(0), barrier, agent-scope
// ticket); the last workgroup sums row[b] and w[y_b] in row order and writes loss and the
// denominator, which the backward reads instead of recounting.  none: no hand-off at all.
// S[b] is saved beside lse[b]: the backward would otherwise need a wave reduction over a[c]
// before its first store.  A row that is not counted never reads w or U (U is indexed by y).
namespace {

struct CeOpt {
    const float* w;  // [C] or nullptr (all ones)
    const float* U;  // [C][ldu] or nullptr (1 / C)
    int64_t ldu;
    float eps, ome, inv_c;  // ome = 1 - eps
};

__device__ __forceinline__ float ce_opt_a(const CeOpt& o, const float* __restrict__ urow, int64_t c, int64_t t) {
    const float u = o.eps != 0.f ? (urow ? urow[c] : o.inv_c) : 0.f;
    const float a = (c == t ? o.ome : 0.f) + o.eps * u;
    return o.w ? o.w[c] * a : a;
}

// loss and denominator over the rows, in row order (one wave; sc1 loads of the row losses)
__device__ __forceinline__ void ce_opt_reduce_wave(float* rowloss, const int64_t* __restrict__ target,
                                                   const float* __restrict__ w, int64_t B, int64_t C, int64_t ignore,
                                                   int reduction, float* __restrict__ loss, float* __restrict__ denom) {
    const int lane = threadIdx.x & 63;
    float acc = 0.f, den = 0.f;
    for (int64_t b0 = 0; b0 < B; b0 += 64) {
        const int64_t b = b0 + lane;
        float v = 0.f, d = 0.f;
        if (b < B) {
            v = __hip_atomic_load(rowloss + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int64_t t = target[b];
            if (t != ignore && t >= 0 && t < C) d = w ? w[t] : 1.f;
        }
        acc += wave_sum(v);
        den += wave_sum(d);
    }
    if (lane == 0) {
        denom[0] = den;
        loss[0] = reduction == 0 ? acc / den : acc;  // mean: NaN when no row is counted, as torch
    }
}

__global__ void __launch_bounds__(kCeThreads)
k_ce_opt_fwd(const float* __restrict__ x, const int64_t* __restrict__ target, int64_t B, int64_t C, int64_t ldx,
             int64_t ignore, CeOpt o, int reduction, float* __restrict__ lse, float* rowloss,
             float* __restrict__ rowsum, unsigned* counter, float* __restrict__ loss, float* __restrict__ denom) {
    __shared__ unsigned is_last;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t b = static_cast<int64_t>(blockIdx.x) * kCeWaves + w; b < B; b += static_cast<int64_t>(gridDim.x) * kCeWaves) {
        const float* row = x + b * ldx;
        const int64_t t = target[b];
        const bool counted = t != ignore && t >= 0 && t < C;  // the same in every lane
        const float* urow = (counted && o.U) ? o.U + t * o.ldu : nullptr;
        float m = -__builtin_huge_valf(), s = 0.f, S = 0.f, acc = 0.f, ls, l;
        if (C <= 64 * kCePer) {
            float v[kCePer];
#pragma unroll
            for (int k = 0; k < kCePer; ++k) {
                const int64_t c = lane + 64 * k;
                v[k] = c < C ? row[c] : -__builtin_huge_valf();
            }
#pragma unroll
            for (int k = 0; k < kCePer; ++k) m = fmaxf(m, v[k]);
            m = wave_max(m);
#pragma unroll
            for (int k = 0; k < kCePer; ++k) s += lane + 64 * k < C ? expf(v[k] - m) : 0.f;
            s = wave_sum(s);
            ls = logf(s);
            l = m + ls;
            if (counted) {
                const float ref = fabsf(l) < kCeLseFine ? l : m;
#pragma unroll
                for (int k = 0; k < kCePer; ++k) {
                    const int64_t c = lane + 64 * k;
                    const float a = c < C ? ce_opt_a(o, urow, c, t) : 0.f;
                    if (a != 0.f) {
                        S += a;
                        acc += a * (ref - v[k]);
                    }
                }
            }
        } else {
            for (int64_t c = lane; c < C; c += 64) m = fmaxf(m, row[c]);
            m = wave_max(m);
            for (int64_t c = lane; c < C; c += 64) s += expf(row[c] - m);
            s = wave_sum(s);
            ls = logf(s);
            l = m + ls;
            if (counted) {
                const float ref = fabsf(l) < kCeLseFine ? l : m;
                for (int64_t c = lane; c < C; c += 64) {
                    const float a = ce_opt_a(o, urow, c, t);
                    if (a != 0.f) {
                        S += a;
                        acc += a * (ref - row[c]);
                    }
                }
            }
        }
        S = wave_sum(S);
        acc = wave_sum(acc);
        if (lane == 0) {
            // a target outside [0, C) other than ignore_index poisons the loss with NaN
            float rl = t == ignore ? 0.f : __builtin_nanf("");
            if (counted) rl = fabsf(l) < kCeLseFine ? acc : S * ls + acc;
            lse[b] = l;
            rowsum[b] = S;
            __hip_atomic_store(rowloss + b, rl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (reduction == 2) return;  // none: the row losses are the result (the same in every workgroup)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's row losses have left
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned old = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        is_last = old + 1 == gridDim.x ? 1u : 0u;
    }
    __syncthreads();
    if (!is_last) return;
    if (w == 0) ce_opt_reduce_wave(rowloss, target, o.w, B, C, ignore, reduction, loss, denom);
    if (threadIdx.x == 0) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(kCeThreads)
k_ce_opt_bwd(const float* __restrict__ x, const int64_t* __restrict__ target, const float* __restrict__ lse,
             const float* __restrict__ rowsum, const float* __restrict__ denom, const float* __restrict__ gout,
             int64_t B, int64_t C, int64_t ldx, int64_t ignore, CeOpt o, int reduction, float* __restrict__ dx,
             int64_t ldd) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float g = reduction == 2 ? 0.f : (reduction == 0 ? gout[0] / denom[0] : gout[0]);
    for (int64_t b = static_cast<int64_t>(blockIdx.x) * kCeWaves + w; b < B; b += static_cast<int64_t>(gridDim.x) * kCeWaves) {
        const float* row = x + b * ldx;
        float* drow = dx + b * ldd;
        const int64_t t = target[b];
        if (!(t != ignore && t >= 0 && t < C)) {  // not counted (the same in every lane): exactly 0
            for (int64_t c = lane; c < C; c += 64) drow[c] = 0.f;
            continue;
        }
        const float* urow = o.U ? o.U + t * o.ldu : nullptr;
        const float G = reduction == 2 ? gout[b] : g;
        const float l = lse[b], S = rowsum[b];
        const bool fine = fabsf(l) < kCeLseFine;
        if (C <= 64 * kCePer) {
            float v[kCePer];
#pragma unroll
            for (int k = 0; k < kCePer; ++k) {
                const int64_t c = lane + 64 * k;
                v[k] = c < C ? row[c] : 0.f;
            }
            float rs = 1.f;
            if (fine) {
#pragma unroll
                for (int k = 0; k < kCePer; ++k) v[k] = expf(v[k] - l);
            } else {
                float m = -__builtin_huge_valf(), s = 0.f;
#pragma unroll
                for (int k = 0; k < kCePer; ++k) m = lane + 64 * k < C ? fmaxf(m, v[k]) : m;
                m = wave_max(m);
#pragma unroll
                for (int k = 0; k < kCePer; ++k) {
                    v[k] = lane + 64 * k < C ? expf(v[k] - m) : 0.f;
                    s += v[k];
                }
                rs = 1.f / wave_sum(s);
            }
#pragma unroll
            for (int k = 0; k < kCePer; ++k) {
                const int64_t c = lane + 64 * k;
                if (c < C) drow[c] = G * (S * (fine ? v[k] : v[k] * rs) - ce_opt_a(o, urow, c, t));
            }
        } else if (fine) {
            for (int64_t c = lane; c < C; c += 64) drow[c] = G * (S * expf(row[c] - l) - ce_opt_a(o, urow, c, t));
        } else {
            float m = -__builtin_huge_valf(), s = 0.f;
            for (int64_t c = lane; c < C; c += 64) m = fmaxf(m, row[c]);
            m = wave_max(m);
            for (int64_t c = lane; c < C; c += 64) s += expf(row[c] - m);
            const float rs = 1.f / wave_sum(s);
            for (int64_t c = lane; c < C; c += 64)
                drow[c] = G * (S * (expf(row[c] - m) * rs) - ce_opt_a(o, urow, c, t));
        }
    }
}

bool ce_opt_args_ok(int64_t B, int64_t C, int64_t ldx, const float* smoothing, int64_t ldu, float eps, int reduction) {
    return B >= 0 && C > 0 && ldx >= C && eps >= 0.f && eps < 1.f && (!smoothing || ldu >= C) && reduction >= 0 &&
           reduction <= 2;
}

CeOpt ce_opt_of(const float* weight, const float* smoothing, int64_t ldu, float eps, int64_t C) {
    return CeOpt{weight, smoothing, ldu, eps, 1.f - eps, 1.f / static_cast<float>(C)};
}

}  // namespace

extern "C" int lg_cross_entropy_opt_fwd(const float* logits, const int64_t* target, int64_t B, int64_t C, int64_t ldx,
                                        int64_t ignore_index, const float* weight, const float* smoothing, int64_t ldu,
                                        float eps, int reduction, float* loss, float* lse, float* rowloss,
                                        float* rowsum, float* denom, unsigned* counter, lg_stream_t stream) {
    if (!ce_opt_args_ok(B, C, ldx, smoothing, ldu, eps, reduction)) return LG_EINVAL;
    if (reduction != 2 && (!loss || !denom || !counter)) return LG_EINVAL;
    if (B > 0 && (!logits || !target || !lse || !rowloss || !rowsum)) return LG_EINVAL;
    hipStream_t s = lg_stream(stream);
    if (B == 0) {  // mean over no rows: NaN (torch); sum: 0; none: nothing to write.  Memset nodes: capturable
        if (reduction == 2) return LG_OK;
        if (hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(loss), reduction == 0 ? 0x7FC00000 : 0, 1, s) != hipSuccess)
            return LG_EHIP;
        return hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(denom), 0, 1, s) == hipSuccess ? LG_OK : LG_EHIP;
    }
    // the grid of lg_cross_entropy_fwd: at most one workgroup per CU (the hand-off's validated grid)
    const int grid = static_cast<int>(std::min<int64_t>((B + kCeWaves - 1) / kCeWaves, lg_num_cus()));
    lg_launch(k_ce_opt_fwd, grid, kCeThreads, 0, s, logits, target, B, C, ldx, ignore_index,
              ce_opt_of(weight, smoothing, ldu, eps, C), reduction, lse, rowloss, rowsum, counter, loss, denom);
    LG_RET_IF_LAUNCH_FAILED();
    return LG_OK;
}

extern "C" int lg_cross_entropy_opt_bwd(const float* logits, const int64_t* target, const float* lse,
                                        const float* rowsum, const float* denom, const float* grad, int64_t B,
                                        int64_t C, int64_t ldx, int64_t ignore_index, const float* weight,
                                        const float* smoothing, int64_t ldu, float eps, int reduction, float* dlogits,
                                        int64_t ldd, lg_stream_t stream) {
    if (!ce_opt_args_ok(B, C, ldx, smoothing, ldu, eps, reduction) || ldd < C) return LG_EINVAL;
    if (reduction == 0 && !denom) return LG_EINVAL;
    if (reduction != 2 && !grad) return LG_EINVAL;
    if (B == 0) return LG_OK;
    if (!logits || !target || !lse || !rowsum || !grad || !dlogits) return LG_EINVAL;
    hipStream_t s = lg_stream(stream);
    const int grid = static_cast<int>(std::min<int64_t>((B + kCeWaves - 1) / kCeWaves, 4 * lg_num_cus()));
    lg_launch(k_ce_opt_bwd, grid, kCeThreads, 0, s, logits, target, lse, rowsum, denom, grad, B, C, ldx, ignore_index,
              ce_opt_of(weight, smoothing, ldu, eps, C), reduction, dlogits, ldd);
    LG_RET_IF_LAUNCH_FAILED();
    return LG_OK;
}
