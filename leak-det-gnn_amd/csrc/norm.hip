// LayerNorm over the feature axis for the pre-norm residual trunk (include/leakgnn.h:
// lg_add_layernorm_fwd, lg_layernorm_bwd).  Rows are D contiguous floats, D in {32, 64}.
//
// Shape of both kernels: wave64, one row per D/4 lanes, each lane one float4 of the row, so a
// wave's loads and stores are 1 KB contiguous (4 rows at D = 64, 8 at D = 32).  The in-row sums
// are DPP butterflies in a fixed order (xor 1, xor 2, mirror within 8, mirror within 16): every
// lane of a row ends with the same bits.  The workgroups walk the row groups in a grid-stride
// loop whose bounds are wave-uniform: in the ragged last group the lanes past the end load
// zeros and store nothing, but stay in the cross-lane sums.  The streaming loop touches no LDS;
// the backward folds its four waves' column sums through 2 KB of LDS once, after the loop.
#include <algorithm>

#include "common.h"
#include "reduce.h"

namespace {

constexpr int kLnWaves = 4;  // waves per workgroup

template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
// sum over the LPR (8 or 16) adjacent lanes that hold one row; the same bits in each of them
template <int LPR>
__device__ __forceinline__ float row_sum(float v) {
    v = dpp_add<0xB1>(v);   // quad_perm [1, 0, 3, 2]: lane ^ 1
    v = dpp_add<0x4E>(v);   // quad_perm [2, 3, 0, 1]: lane ^ 2
    v = dpp_add<0x141>(v);  // row_half_mirror: lane 7 - i of each 8
    if constexpr (LPR == 16) v = dpp_add<0x140>(v);  // row_mirror: lane 15 - i of each 16
    return v;
}
__device__ __forceinline__ float sum4(f32x4 v) { return (v[0] + v[1]) + (v[2] + v[3]); }

// xsum = x + f (ADD), xn = (xsum - mean) * rstd * gamma + beta, stats = (mean, rstd) (STATS).
// Two passes over the row in registers: the mean, then the squared distances from it.
template <int D, bool ADD, bool STATS>
__global__ void __launch_bounds__(64 * kLnWaves)
k_add_ln_fwd(const float* __restrict__ x, const float* __restrict__ f, const float* __restrict__ gamma,
             const float* __restrict__ beta, float* __restrict__ xsum, float* __restrict__ xn,
             float* __restrict__ stats, int64_t rows, float eps) {
    // no fused multiply-add: every instantiation rounds the same expression the same way (the
    // entry norm of x == the call with f = zeros, bit for bit)
#pragma clang fp contract(off)
    constexpr int LPR = D / 4, RPW = 64 / LPR;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c4 = 4 * (lane % LPR), rin = lane / LPR;
    const f32x4 gam = ld4(gamma + c4), bet = ld4(beta + c4);
    const int64_t ngroups = (rows + RPW - 1) / RPW;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int64_t g = static_cast<int64_t>(blockIdx.x) * kLnWaves + wave; g < ngroups;
         g += static_cast<int64_t>(gridDim.x) * kLnWaves) {
        const int64_t row = g * RPW + rin;
        const bool ok = row < rows;
        const int64_t off = row * D + c4;
        f32x4 v = ok ? ld4(x + off) : zero;
        if constexpr (ADD) {
            const f32x4 fv = ok ? ld4(f + off) : zero;
            v = v + fv;  // one fp32 add per element, nothing to contract it with
            if (ok) st4(xsum + off, v);
        }
        const float mean = row_sum<LPR>(sum4(v)) * (1.0f / D);
        const f32x4 d = v - mean;
        const float var = row_sum<LPR>(sum4(d * d)) * (1.0f / D);
        const float rstd = 1.0f / sqrtf(var + eps);
        if (ok) {
            st4(xn + off, d * rstd * gam + bet);
            if constexpr (STATS) {
                if (c4 == 0) *reinterpret_cast<float2*>(stats + 2 * row) = make_float2(mean, rstd);
            }
        }
    }
}

// dx = rstd * (g - mean(g) - xhat * mean(g * xhat)), g = dxn * gamma; + carry (CARRY); then
// * scale_out * [x > 0] (MASK).  Each lane keeps its four columns' sums of dxn * xhat and dxn over
// the rows it visits; after the loop they are folded over the wave's row slots (xor shuffles),
// then over the four waves in wave order, into slab[blockIdx][0 .. D) (dgamma) and [D .. 2 D).
template <int D, bool CARRY, bool MASK>
__global__ void __launch_bounds__(64 * kLnWaves)
k_ln_bwd(const float* __restrict__ dxn, const float* __restrict__ x, const float* __restrict__ stats,
         const float* __restrict__ gamma, const float* carry, float* dx_out, float* __restrict__ slab, int64_t rows,
         float scale_out) {
    // no fused multiply-add in this kernel: the carry's add and the mask's scale must stay
    // roundings of their own after the products before them (dx with the carry == dx without
    // it + carry, bit for bit, in every instantiation)
#pragma clang fp contract(off)
    constexpr int LPR = D / 4, RPW = 64 / LPR;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c4 = 4 * (lane % LPR), rin = lane / LPR;
    const f32x4 gam = ld4(gamma + c4);
    const int64_t ngroups = (rows + RPW - 1) / RPW;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 ag = zero, ab = zero;
    for (int64_t g = static_cast<int64_t>(blockIdx.x) * kLnWaves + wave; g < ngroups;
         g += static_cast<int64_t>(gridDim.x) * kLnWaves) {
        const int64_t row = g * RPW + rin;
        const bool ok = row < rows;
        const int64_t off = row * D + c4;
        const f32x4 dv = ok ? ld4(dxn + off) : zero;
        const f32x4 xv = ok ? ld4(x + off) : zero;
        const float2 ms = ok ? *reinterpret_cast<const float2*>(stats + 2 * row) : make_float2(0.f, 0.f);
        f32x4 cv = zero;
        if constexpr (CARRY) cv = ok ? ld4(carry + off) : zero;
        const f32x4 xh = (xv - ms.x) * ms.y;
        const f32x4 gv = dv * gam;
        const float m1 = row_sum<LPR>(sum4(gv)) * (1.0f / D);
        const float m2 = row_sum<LPR>(sum4(gv * xh)) * (1.0f / D);
        f32x4 dx = (gv - m1 - xh * m2) * ms.y;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if constexpr (CARRY) dx[i] = dx[i] + cv[i];
            if constexpr (MASK) dx[i] = xv[i] > 0.f ? dx[i] * scale_out : 0.f;
        }
        if (ok) st4(dx_out + off, dx);
        ag += dv * xh;  // rows past the end: dv = 0
        ab += dv;
    }
    __shared__ float part[kLnWaves][2 * D];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int o = 32; o >= LPR; o >>= 1) {
            ag[i] += __shfl_xor(ag[i], o);
            ab[i] += __shfl_xor(ab[i], o);
        }
    }
    if (rin == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            part[wave][c4 + i] = ag[i];
            part[wave][D + c4 + i] = ab[i];
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * D) {
        float t = part[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kLnWaves; ++w) t += part[w][threadIdx.x];
        slab[static_cast<int64_t>(blockIdx.x) * (2 * D) + threadIdx.x] = t;
    }
}

int ln_grid(int64_t rows, int64_t D, int per_cu) {
    const int64_t rpw = 64 / (D / 4);
    const int64_t need = ((rows + rpw - 1) / rpw + kLnWaves - 1) / kLnWaves;
    return static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(need, static_cast<int64_t>(per_cu) * lg_num_cus())));
}

constexpr int kLnBwdBlocksPerCu = 2;  // slab rows: 2 x CUs, as the trunk backward's

}  // namespace

extern "C" int lg_add_layernorm_fwd(const float* x, const float* f, const float* gamma, const float* beta, float* xsum,
                                    float* xn, float* stats, int64_t rows, int64_t D, float eps, lg_stream_t stream) {
    if (!x || !xn || !gamma || !beta || rows < 0 || !(eps >= 0.f)) return LG_EINVAL;
    if ((f == nullptr) != (xsum == nullptr)) return LG_EINVAL;
    if (D != 32 && D != 64) return LG_EUNSUPPORTED;
    if (rows >= kLgMaxRows) return LG_EUNSUPPORTED;
    if (rows == 0) return LG_OK;
    hipStream_t s = lg_stream(stream);
    const int grid = ln_grid(rows, D, 4);
    auto launch = [&](auto kern) { lg_launch(kern, grid, 64 * kLnWaves, 0, s, x, f, gamma, beta, xsum, xn, stats, rows, eps); };
#define LG_LN_FWD(DD)                                            \
    do {                                                         \
        if (f) {                                                 \
            if (stats) launch(k_add_ln_fwd<DD, true, true>);     \
            else launch(k_add_ln_fwd<DD, true, false>);          \
        } else {                                                 \
            if (stats) launch(k_add_ln_fwd<DD, false, true>);    \
            else launch(k_add_ln_fwd<DD, false, false>);         \
        }                                                        \
    } while (0)
    if (D == 64) LG_LN_FWD(64);
    else LG_LN_FWD(32);
#undef LG_LN_FWD
    LG_RET_IF_LAUNCH_FAILED();
    return LG_OK;
}

extern "C" int64_t lg_layernorm_bwd_workspace_bytes(int64_t D) {
    if (D != 32 && D != 64) return LG_EUNSUPPORTED;
    return static_cast<int64_t>(kLnBwdBlocksPerCu) * lg_num_cus() * 2 * D * static_cast<int64_t>(sizeof(float));
}

extern "C" int lg_layernorm_bwd(const float* dxn, const float* x, const float* stats, const float* gamma,
                                const float* carry, float* dx_out, float* dgamma, float* dbeta, int64_t rows, int64_t D,
                                int flags, float scale_out, void* workspace, int64_t ws_bytes, lg_stream_t stream) {
    if (!dxn || !x || !stats || !gamma || !dx_out || !dgamma || !dbeta || !workspace || rows < 0) return LG_EINVAL;
    if (flags & ~LG_F_MASK_OUT) return LG_EUNSUPPORTED;
    if (D != 32 && D != 64) return LG_EUNSUPPORTED;
    if (rows >= kLgMaxRows) return LG_EUNSUPPORTED;
    if (ws_bytes < lg_layernorm_bwd_workspace_bytes(D)) return LG_EINVAL;
    hipStream_t s = lg_stream(stream);
    float* slab = static_cast<float*>(workspace);
    // rows == 0 still runs one (empty) workgroup so the slab holds zeros
    const int grid = ln_grid(rows, D, kLnBwdBlocksPerCu);
    const bool mask = (flags & LG_F_MASK_OUT) != 0;
    auto launch = [&](auto kern) {
        lg_launch(kern, grid, 64 * kLnWaves, 0, s, dxn, x, stats, gamma, carry, dx_out, slab, rows, scale_out);
    };
#define LG_LN_BWD(DD)                                         \
    do {                                                      \
        if (carry) {                                          \
            if (mask) launch(k_ln_bwd<DD, true, true>);       \
            else launch(k_ln_bwd<DD, true, false>);           \
        } else {                                              \
            if (mask) launch(k_ln_bwd<DD, false, true>);      \
            else launch(k_ln_bwd<DD, false, false>);          \
        }                                                     \
    } while (0)
    if (D == 64) LG_LN_BWD(64);
    else LG_LN_BWD(32);
#undef LG_LN_BWD
    LG_RET_IF_LAUNCH_FAILED();
    const LgSlabSeg segs[2] = {{0, D, dgamma}, {D, D, dbeta}};
    return lg_launch_slab_reduce_multi(slab, grid, 2 * D, segs, 2, nullptr, nullptr, s);
}
