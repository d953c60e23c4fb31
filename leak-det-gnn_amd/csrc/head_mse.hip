// The predictor's training tail (reference train_predictor.py: nn.MSELoss() over the output of
// head = nn.Linear(H, S) on the last hidden state), forward and backward.  torch runs it as about
// eight launches for 1.9 MFLOP at the CLI's shape (addmm, sub, pow, mean, their backwards, two
// GEMMs and a column sum); here:
//   forward : y_hat = h W^T + b, one wave per row b: the lanes split H (coalesced W rows, the row
//             of h in registers), a fixed shuffle tree per output, lane s % 64 keeps output s and
//             adds the bias.  W is staged in LDS when S * H floats fit kHmLdsFloats, else every
//             wave reads it through L2.  Each row's sum of (y_hat - y)^2 goes to rowsq[b]; the
//             workgroup that finishes last sums the rows in row order (fp64) in the same launch,
//             by k_ce_fwd's fence-free hand-off (loss.hip: sc1 stores, vmcnt(0), a workgroup
//             barrier, one agent-scope ticket; at most one workgroup per CU, so all are resident).
//   backward: d = 2 g / (B S) (y_hat - y); dh = d W by one wave per row; [dW | db] = [d^T h | sum_b d]
//             as one partial per chunk of rows (each thread owns columns, sums its chunk's rows in
//             row order), reduced by reduce.hip's fixed-order fp64 slab reduction.  No atomics on
//             floats: two runs give the same bits.  Every output element is written.
// Plain fp32 FMA: the pair is launch-bound (no throughput is claimed for it).
#include <algorithm>
#include "common.h"
#include "reduce.h"

namespace {

constexpr int kHmWaves = 4;
constexpr int kHmThreads = 64 * kHmWaves;
constexpr int kHmPer = 16;                    // row elements per lane held in registers (H <= 1024)
constexpr int64_t kHmMaxDim = 64 * kHmPer;    // largest H and S
constexpr int64_t kHmLdsFloats = 39 * 1024;   // W is staged in LDS up to this many floats (156 KB)
static_assert(kHmLdsFloats * 4 + 1024 <= 160 * 1024, "LDS budget: staged W + the kernel's static words");
constexpr int kHmTile = kHmThreads * 16;      // backward: [dW | db] columns per workgroup
constexpr int kHmMaxChunks = 256;             // backward: most row chunks (= slab rows)
constexpr int64_t kHmSlabFloats = int64_t{1} << 24;  // backward: most partial floats (64 MB)

__device__ __forceinline__ float hm_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double hm_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <bool kLds>
__global__ void __launch_bounds__(kHmThreads)
k_head_mse_fwd(const float* __restrict__ h, const float* __restrict__ W, const float* __restrict__ bias,
               const float* __restrict__ y, int64_t B, int H, int S, float* __restrict__ yhat, float* rowsq,
               unsigned* counter, float* __restrict__ loss) {
    extern __shared__ __attribute__((aligned(16))) float wl[];  // kLds: W (S, H)
    __shared__ unsigned is_last;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (kLds) {
        const int n = S * H, n4 = n >> 2;  // W's base is 16-byte aligned (checked by the host)
        for (int i = threadIdx.x; i < n4; i += kHmThreads) st4(wl + 4 * i, ld4(W + 4 * i));
        for (int i = 4 * n4 + threadIdx.x; i < n; i += kHmThreads) wl[i] = W[i];
        __syncthreads();
    }
    const int nk = (H + 63) >> 6;
    for (int64_t b = static_cast<int64_t>(blockIdx.x) * kHmWaves + w; b < B; b += static_cast<int64_t>(gridDim.x) * kHmWaves) {
        float hv[kHmPer];
#pragma unroll
        for (int k = 0; k < kHmPer; ++k) {
            const int c = lane + 64 * k;
            hv[k] = c < H ? h[b * H + c] : 0.f;
        }
        float sq = 0.f;
        for (int s0 = 0; s0 < S; s0 += 64) {
            const int ns = min(64, S - s0);
            float mine = 0.f;
            for (int j = 0; j < ns; ++j) {
                const int64_t base = static_cast<int64_t>(s0 + j) * H;
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < kHmPer; ++k) {
                    if (k < nk) {
                        const int c = lane + 64 * k;
                        float wv = 0.f;
                        if (c < H) {
                            if constexpr (kLds) wv = wl[base + c];
                            else wv = W[base + c];
                        }
                        acc = fmaf(hv[k], wv, acc);
                    }
                }
                acc = hm_wave_sum(acc);  // the same bits in every lane
                if (lane == j) mine = acc;
            }
            const int s = s0 + lane;
            if (s < S) {
                const float yh = mine + bias[s];
                yhat[b * S + s] = yh;
                const float d = yh - y[b * S + s];
                sq = fmaf(d, d, sq);
            }
        }
        sq = hm_wave_sum(sq);
        if (lane == 0) __hip_atomic_store(rowsq + b, sq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's row sums have left
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned old = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        is_last = old + 1 == gridDim.x ? 1u : 0u;
    }
    __syncthreads();
    if (!is_last) return;
    if (w == 0) {  // the mean, rows in order (sc1 loads: other workgroups of this launch stored them sc1)
        double acc = 0.0;
        for (int64_t b0 = 0; b0 < B; b0 += 64) {
            const int64_t b = b0 + lane;
            const float v = b < B ? __hip_atomic_load(rowsq + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
            acc += hm_wave_sum(static_cast<double>(v));
        }
        if (lane == 0) loss[0] = static_cast<float>(acc / (static_cast<double>(B) * S));
    }
    if (threadIdx.x == 0) __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// blockIdx.x: chunk of rpc rows; blockIdx.y: tile of kHmTile columns of [dW (S * H) | db (S)]
__global__ void __launch_bounds__(kHmThreads)
k_head_mse_bwd(const float* __restrict__ h, const float* __restrict__ W, const float* __restrict__ y,
               const float* __restrict__ yhat, const float* __restrict__ gout, int64_t B, int H, int S, int64_t rpc,
               float* __restrict__ dh, float* __restrict__ slab) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float c = 2.f * gout[0] / (static_cast<float>(B) * static_cast<float>(S));
    const int64_t r0 = static_cast<int64_t>(blockIdx.x) * rpc, r1 = min(B, r0 + rpc);
    if (blockIdx.y == 0) {  // dh of the chunk's rows: one wave per row, the lanes split H
        const int nk = (H + 63) >> 6;
        for (int64_t b = r0 + w; b < r1; b += kHmWaves) {
            float acc[kHmPer];
#pragma unroll
            for (int k = 0; k < kHmPer; ++k) acc[k] = 0.f;
            for (int s0 = 0; s0 < S; s0 += 64) {
                const int ns = min(64, S - s0);
                const int s = s0 + lane;
                const float dl = s < S ? c * (yhat[b * S + s] - y[b * S + s]) : 0.f;
                for (int j = 0; j < ns; ++j) {
                    const float ds = __shfl(dl, j);
                    const float* wr = W + static_cast<int64_t>(s0 + j) * H;
#pragma unroll
                    for (int k = 0; k < kHmPer; ++k) {
                        const int cc = lane + 64 * k;
                        if (k < nk && cc < H) acc[k] = fmaf(ds, wr[cc], acc[k]);
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < kHmPer; ++k) {
                const int cc = lane + 64 * k;
                if (cc < H) dh[b * H + cc] = acc[k];
            }
        }
    }
    const int64_t nw = static_cast<int64_t>(S) * H, cols = nw + S;
    float* out = slab + static_cast<int64_t>(blockIdx.x) * cols;
    for (int j = 0; j < kHmTile / kHmThreads; ++j) {
        const int64_t col = static_cast<int64_t>(blockIdx.y) * kHmTile + j * kHmThreads + threadIdx.x;
        if (col >= cols) break;
        const bool isb = col >= nw;
        const int s = isb ? static_cast<int>(col - nw) : static_cast<int>(col / H);
        const int hh = isb ? 0 : static_cast<int>(col - static_cast<int64_t>(s) * H);
        float acc = 0.f;
        for (int64_t b = r0; b < r1; ++b) {
            const float d = c * (yhat[b * S + s] - y[b * S + s]);
            acc = isb ? acc + d : fmaf(d, h[b * H + hh], acc);
        }
        out[col] = acc;
    }
}

bool hm_dims_ok(int64_t B, int64_t H, int64_t S) {
    return B >= 1 && H >= 1 && H <= kHmMaxDim && S >= 1 && S <= kHmMaxDim &&
           B * std::max(H, S) * 4 < (int64_t{1} << 31);
}

// rows per chunk and chunk count of the backward's partials (a function of the shape alone)
void hm_chunks(int64_t B, int64_t H, int64_t S, int64_t* rpc, int* chunks) {
    const int64_t cols = S * H + S;
    int64_t n = std::min<int64_t>((B + kHmWaves - 1) / kHmWaves, kHmMaxChunks);
    n = std::max<int64_t>(1, std::min<int64_t>(n, kHmSlabFloats / cols));
    *rpc = (B + n - 1) / n;
    *chunks = static_cast<int>((B + *rpc - 1) / *rpc);
}

}  // namespace

extern "C" int lg_head_mse_fwd(const float* h, const float* weight, const float* bias, const float* target, int64_t B,
                               int64_t H, int64_t S, float* y_hat, float* rowsq, float* loss, unsigned* counter,
                               lg_stream_t stream) {
    if (!h || !weight || !bias || !target || !y_hat || !rowsq || !loss || !counter || !hm_dims_ok(B, H, S))
        return LG_EINVAL;
    hipStream_t s = lg_stream(stream);
    // at most one workgroup per CU: all resident, as k_ce_fwd's hand-off needs; larger B loops
    const int grid = static_cast<int>(std::min<int64_t>((B + kHmWaves - 1) / kHmWaves, lg_num_cus()));
    const int Hi = static_cast<int>(H), Si = static_cast<int>(S);
    const bool lds = S * H <= kHmLdsFloats && (reinterpret_cast<uintptr_t>(weight) & 15u) == 0;
    if (lds) {
        const int64_t dyn = S * H * 4;
        if (dyn > 64 * 1024 &&
            hipFuncSetAttribute(reinterpret_cast<const void*>(k_head_mse_fwd<true>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(dyn)) != hipSuccess)
            return LG_EHIP;
        lg_launch(k_head_mse_fwd<true>, grid, kHmThreads, static_cast<uint32_t>(dyn), s, h, weight, bias, target, B, Hi,
                  Si, y_hat, rowsq, counter, loss);
    } else {
        lg_launch(k_head_mse_fwd<false>, grid, kHmThreads, 0, s, h, weight, bias, target, B, Hi, Si, y_hat, rowsq,
                  counter, loss);
    }
    LG_RET_IF_LAUNCH_FAILED();
    return LG_OK;
}

extern "C" int64_t lg_head_mse_bwd_workspace_bytes(int64_t B, int64_t H, int64_t S) {
    if (!hm_dims_ok(B, H, S)) return LG_EINVAL;
    int64_t rpc;
    int chunks;
    hm_chunks(B, H, S, &rpc, &chunks);
    return chunks * (S * H + S) * 4;
}

extern "C" int lg_head_mse_bwd(const float* h, const float* weight, const float* target, const float* y_hat,
                               const float* grad_loss, int64_t B, int64_t H, int64_t S, float* dh, float* dweight,
                               float* dbias, void* workspace, int64_t ws_bytes, lg_stream_t stream) {
    if (!h || !weight || !target || !y_hat || !grad_loss || !dh || !dweight || !dbias || !workspace ||
        !hm_dims_ok(B, H, S))
        return LG_EINVAL;
    int64_t rpc;
    int chunks;
    hm_chunks(B, H, S, &rpc, &chunks);
    const int64_t cols = S * H + S;
    if (ws_bytes < chunks * cols * 4) return LG_EINVAL;
    hipStream_t s = lg_stream(stream);
    float* slab = static_cast<float*>(workspace);
    const dim3 grid(chunks, static_cast<unsigned>((cols + kHmTile - 1) / kHmTile));
    lg_launch(k_head_mse_bwd, grid, kHmThreads, 0, s, h, weight, target, y_hat, grad_loss, B, static_cast<int>(H),
              static_cast<int>(S), rpc, dh, slab);
    LG_RET_IF_LAUNCH_FAILED();
    const LgSlabSeg segs[2] = {LgSlabSeg{0, S * H, dweight}, LgSlabSeg{S * H, S, dbias}};
    return lg_launch_slab_reduce_multi(slab, chunks, cols, segs, 2, nullptr, nullptr, s);
}
