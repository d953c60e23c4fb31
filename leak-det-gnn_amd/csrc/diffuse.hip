// K-hop diffusion of the node init (APPNP's personalised-PageRank propagation; include/leakgnn.h:
// lg_diffuse_fwd, lg_diffuse_bwd).  Node-major [N][B][D] fp32, Ahat from the node tables of
// lg_nm_table_build (records 0 .. N-1, node order; self loop and edge weights included).
//
//   forward:   z_0 = x_0,  z_{k+1} = (1 - alpha) Ahat z_k + alpha x_0
//   backward:  u = g, acc = 0;  K times: acc += alpha u, u = (1 - alpha) Ahat^T u;  dx_0 = u + acc
//
// Every window and every channel propagates on its own, so there are two forms of each pass:
//
//   resident (k_diffuse_res): ONE launch runs all K hops.  A workgroup owns one window and a
//     channel slice of CS = 32, 16 or 8 floats: the slice's N rows sit in ONE LDS buffer of
//     N * CS * 4 bytes, row n at float n * CS (CS / 4 lanes per row, one float4 each).  A thread
//     owns rows rp, rp + RPP, ... (RPP = threads / (CS / 4)) and keeps two float4 per owned row in
//     registers across the hops: the row's current value and alpha * x_0 (forward) or acc
//     (backward).  512 threads x at most 12 rows: 96 of a thread's 256 VGPRs hold rows (1024
//     threads x 6 rows spill at 128 VGPRs, 512 x 20 at 256), so a slice holds N <= 12 * RPP rows:
//     768, 1536, 3072 at CS = 32, 16, 8 (98 KB of LDS at most).  A hop: every thread sums its rows'
//     neighbours out of LDS into registers, barrier, writes its rows back, barrier.  x_0 is read from HBM once
//     and z_K written once, whatever K is.  No atomics, no polls, no hand-off between workgroups.
//     LDS reads: a ds_read_b128 lane group is 16 lanes, i.e. (at CS = 32) four 64-byte half rows
//     of four different rows; neighbour rows sit at arbitrary offsets, so no row layout makes every
//     group conflict-free (two of the four collide when their rows have the same parity: 2-way).
//     The plain [row][CS] image keeps the 8 (4, 2) lanes of one row on one contiguous 128 (64,
//     32) bytes, which is the part a layout can give.
//   hop-wise (k_diffuse_hop): one launch per hop, ping-pong in HBM (the caller's workspace), any N.
//
// Both forms sum a row's entries in the record's CSR order (the six inline pairs, then the
// overflow pairs) through the same device functions with contraction off, so they give the same
// bits (tests/test_gpu_diffuse.py).
#include <algorithm>

#include "common.h"

namespace {

constexpr int kDfThreads = 512;             // resident workgroup (8 waves)
constexpr int kDfRows = 12;                 // rows a resident thread owns at most
constexpr int kDfLdsBytes = 160 * 1024;     // LDS of a gfx950 CU
constexpr int kDfHopThreads = 256;
constexpr bool kDfResidentDefault = true;   // the form a graph that fits takes without LG_F_DIFFUSE_HOPWISE

// every slice's rows at kDfRows per thread are the same kDfRows * kDfThreads * 16 bytes of LDS
static_assert(kDfRows * kDfThreads * 16 <= kDfLdsBytes, "a slice's rows exceed the LDS");

__device__ __forceinline__ float as_f(int v) { return __int_as_float(v); }

// (Ahat z)[row of rec]: s = 0, then s = s + w_k * z[col_k] for the record's entries in CSR order.
// fetch(col) returns the lane's float4 of row col.
template <typename Fetch>
__device__ __forceinline__ f32x4 df_row_sum(const int4* __restrict__ rec, const int2* __restrict__ pairs, Fetch fetch) {
#pragma clang fp contract(off)
    const int4 r0 = rec[0], r1 = rec[1], r2 = rec[2], r3 = rec[3];
    const int e0 = r0.x, e1 = r0.y, cnt = e1 - e0;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (cnt > 0) s = s + as_f(r0.w) * fetch(r0.z);
    if (cnt > 1) s = s + as_f(r1.y) * fetch(r1.x);
    if (cnt > 2) s = s + as_f(r1.w) * fetch(r1.z);
    if (cnt > 3) s = s + as_f(r2.y) * fetch(r2.x);
    if (cnt > 4) s = s + as_f(r2.w) * fetch(r2.z);
    if (cnt > 5) s = s + as_f(r3.y) * fetch(r3.x);
    for (int e = e0 + kLgNmInline; e < e1; ++e) {
        const int2 p = pairs[e];
        s = s + as_f(p.y) * fetch(p.x);
    }
    return s;
}

// the hops' own arithmetic, one rounding per operation
__device__ __forceinline__ f32x4 df_fwd_step(f32x4 s, f32x4 ax0, float oma) {
#pragma clang fp contract(off)
    const f32x4 t = oma * s;
    return t + ax0;
}
__device__ __forceinline__ f32x4 df_scale(f32x4 v, float a) {
#pragma clang fp contract(off)
    return a * v;
}
__device__ __forceinline__ f32x4 df_acc(f32x4 acc, f32x4 u, float alpha) {
#pragma clang fp contract(off)
    const f32x4 t = alpha * u;
    return acc + t;
}
template <bool MASK>
__device__ __forceinline__ f32x4 df_bwd_out(f32x4 u, f32x4 acc, const float* __restrict__ x0row, float scale_out) {
#pragma clang fp contract(off)
    f32x4 dx = u + acc;
    if constexpr (MASK) {
        const f32x4 xv = ld4(x0row);
#pragma unroll
        for (int i = 0; i < 4; ++i) dx[i] = xv[i] > 0.f ? dx[i] * scale_out : 0.f;
    }
    return dx;
}

// All hops in one launch.  blockIdx.x = window * (D / CS) + slice.  in: x_0 (forward) or g
// (backward); x0: the mask's x_0 (MASK).  N <= kDfRows * RPP (host: df_slice).
template <int CS, bool BWD, bool MASK>
__global__ void __launch_bounds__(kDfThreads)
k_diffuse_res(const int4* __restrict__ tab, const int2* __restrict__ pairs, const float* __restrict__ in,
              const float* __restrict__ x0, float* __restrict__ out, int B, int N, int D, int hops, float alpha,
              float scale_out) {
    extern __shared__ __attribute__((aligned(16))) float df_lds[];
    constexpr int LPR = CS / 4, RPP = kDfThreads / LPR, KR = kDfRows;
    const int nsl = D / CS;
    const int b = blockIdx.x / nsl, c0 = (blockIdx.x % nsl) * CS;
    const int c4 = 4 * (threadIdx.x % LPR), rp = threadIdx.x / LPR;
    const float oma = 1.0f - alpha;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 cur[KR], keep[KR];  // the row's value now in LDS; alpha * x_0 (forward) or acc (backward)
    auto goff = [&](int n) { return (static_cast<int64_t>(n) * B + b) * D + c0 + c4; };
#pragma unroll
    for (int i = 0; i < KR; ++i) {
        const int n = rp + RPP * i;
        cur[i] = keep[i] = zero;
        if (n < N) {
            cur[i] = ld4(in + goff(n));
            st4(df_lds + n * CS + c4, cur[i]);
            if constexpr (!BWD) keep[i] = df_scale(cur[i], alpha);
        }
    }
    __syncthreads();
    for (int h = 0; h < hops; ++h) {
#pragma unroll
        for (int i = 0; i < KR; ++i) {
            const int n = rp + RPP * i;
            if (n < N) {
                const f32x4 s = df_row_sum(tab + 4 * n, pairs, [&](int c) { return ld4(df_lds + c * CS + c4); });
                if constexpr (BWD) {
                    keep[i] = df_acc(keep[i], cur[i], alpha);
                    cur[i] = df_scale(s, oma);
                } else {
                    cur[i] = df_fwd_step(s, keep[i], oma);
                }
            }
        }
        if (h + 1 == hops) break;  // (uniform) the last hop's rows leave from registers
        __syncthreads();           // every read of this hop's image is done
#pragma unroll
        for (int i = 0; i < KR; ++i) {
            const int n = rp + RPP * i;
            if (n < N) st4(df_lds + n * CS + c4, cur[i]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < KR; ++i) {
        const int n = rp + RPP * i;
        if (n < N) {
            const int64_t o = goff(n);
            if constexpr (BWD) st4(out + o, df_bwd_out<MASK>(cur[i], keep[i], x0 + o, scale_out));
            else st4(out + o, cur[i]);
        }
    }
}

// One hop.  Row r = n * B + b per D / 4 lanes.  Forward: dst = (1 - alpha) Ahat src + alpha x0.
// Backward: acc' = (first ? 0 : acc) + alpha src, u' = (1 - alpha) Ahat^T src; last: dst = u' + acc'
// (masked under MASK), else dst = u' and acc = acc' (a thread's own element only).
template <int D, bool BWD, bool MASK>
__global__ void __launch_bounds__(kDfHopThreads)
k_diffuse_hop(const int4* __restrict__ tab, const int2* __restrict__ pairs, const float* __restrict__ src,
              const float* __restrict__ x0, float* acc, float* __restrict__ dst, lg_fastdiv divB, int B, int64_t rows,
              float alpha, float scale_out, int first, int last) {
    constexpr int LPR = D / 4;
    const int64_t gid = static_cast<int64_t>(blockIdx.x) * kDfHopThreads + threadIdx.x;
    const int64_t row = gid / LPR;
    if (row >= rows) return;
    const int c4 = 4 * static_cast<int>(gid % LPR);
    const uint32_t n = lg_div(static_cast<uint32_t>(row), divB);
    const uint32_t b = static_cast<uint32_t>(row) - n * static_cast<uint32_t>(B);
    const float oma = 1.0f - alpha;
    const f32x4 s = df_row_sum(tab + 4 * static_cast<int64_t>(n), pairs, [&](int c) {
        return ld4(src + (static_cast<int64_t>(c) * B + b) * D + c4);
    });
    const int64_t o = row * D + c4;
    if constexpr (BWD) {
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        const f32x4 a = df_acc(first ? zero : ld4(acc + o), ld4(src + o), alpha);
        const f32x4 u = df_scale(s, oma);
        if (last) {
            st4(dst + o, df_bwd_out<MASK>(u, a, x0 + o, scale_out));
        } else {
            st4(dst + o, u);
            st4(acc + o, a);
        }
    } else {
        st4(dst + o, df_fwd_step(s, df_scale(ld4(x0 + o), alpha), oma));
    }
}

// the resident form's slice width for an N-node graph: the widest of 32, 16, 8 (and <= D) whose N
// rows fit the LDS budget and kDfRows rows per thread; 0: none fits
int df_slice(int64_t N, int64_t D) {
    for (int cs : {32, 16, 8}) {
        if (cs > D) continue;
        if (N * cs * 4 <= kDfLdsBytes && N <= static_cast<int64_t>(kDfRows) * (kDfThreads / (cs / 4))) return cs;
    }
    return 0;
}

bool df_resident(int64_t N, int64_t D, int flags) {
    return kDfResidentDefault && !(flags & LG_F_DIFFUSE_HOPWISE) && df_slice(N, D) > 0;
}

template <typename Kern>
bool df_allow_lds(Kern kernel, int64_t dyn) {
    return dyn <= 64 * 1024 || hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize,
                                                   static_cast<int>(dyn)) == hipSuccess;
}

template <bool BWD, bool MASK>
int df_launch_res(int cs, const int32_t* tab, const int32_t* pairs, const float* in, const float* x0, float* out,
                  int64_t B, int64_t N, int64_t D, int64_t hops, float alpha, float scale_out, hipStream_t s) {
    const int64_t grid = B * (D / cs), lds = N * cs * 4;
    if (grid >= kLgMaxRows || lds > kDfLdsBytes) return LG_EUNSUPPORTED;
    auto go = [&](auto kern) {
        if (!df_allow_lds(kern, lds)) return static_cast<int>(LG_EHIP);
        lg_launch(kern, static_cast<int>(grid), kDfThreads, static_cast<uint32_t>(lds), s,
                  reinterpret_cast<const int4*>(tab), reinterpret_cast<const int2*>(pairs), in, x0, out,
                  static_cast<int>(B), static_cast<int>(N), static_cast<int>(D), static_cast<int>(hops), alpha, scale_out);
        return static_cast<int>(LG_OK);
    };
    const int rc = cs == 32 ? go(k_diffuse_res<32, BWD, MASK>)
                 : cs == 16 ? go(k_diffuse_res<16, BWD, MASK>) : go(k_diffuse_res<8, BWD, MASK>);
    if (rc != LG_OK) return rc;
    LG_RET_IF_LAUNCH_FAILED();
    return LG_OK;
}

template <bool BWD, bool MASK>
void df_launch_hop(const int32_t* tab, const int32_t* pairs, const float* src, const float* x0, float* acc, float* dst,
                   int64_t B, int64_t N, int64_t D, float alpha, float scale_out, int first, int last, hipStream_t s) {
    const int64_t rows = N * B;
    const int64_t grid = (rows * (D / 4) + kDfHopThreads - 1) / kDfHopThreads;
    const lg_fastdiv divB = lg_make_fastdiv(static_cast<uint32_t>(B));
    auto go = [&](auto kern) {
        lg_launch(kern, static_cast<int>(grid), kDfHopThreads, 0, s, reinterpret_cast<const int4*>(tab),
                  reinterpret_cast<const int2*>(pairs), src, x0, acc, dst, divB, static_cast<int>(B), rows, alpha,
                  scale_out, first, last);
    };
    if (D == 64) go(k_diffuse_hop<64, BWD, MASK>);
    else go(k_diffuse_hop<32, BWD, MASK>);
}

// the checks both entry points share; LG_OK: go on
int df_check(const void* tab, const void* pairs, const void* in, const void* out, int64_t B, int64_t N, int64_t D,
             int64_t hops, float alpha) {
    if (!tab || !pairs || !in || !out || B < 0 || N <= 0 || in == out) return LG_EINVAL;
    if (D != 32 && D != 64) return LG_EUNSUPPORTED;
    if (hops < 1 || hops > 64 || !(alpha >= 0.f && alpha <= 1.f)) return LG_EINVAL;
    if (N > INT32_MAX / 32 || B > INT32_MAX || N * B >= kLgMaxRows) return LG_EUNSUPPORTED;
    return LG_OK;
}

}  // namespace

extern "C" int lg_diffuse_slice(int64_t N, int64_t D) {
    if (N <= 0) return LG_EINVAL;
    if (D != 32 && D != 64) return LG_EUNSUPPORTED;
    return df_slice(N, D);
}

extern "C" int64_t lg_diffuse_workspace_bytes(int64_t B, int64_t N, int64_t D, int64_t hops, int flags, int backward) {
    if (B < 0 || N <= 0 || hops < 1 || hops > 64) return LG_EINVAL;
    if (D != 32 && D != 64) return LG_EUNSUPPORTED;
    if (df_resident(N, D, flags) || hops < 2) return 0;
    return (backward ? 2 : 1) * N * B * D * static_cast<int64_t>(sizeof(float));
}

extern "C" int lg_diffuse_fwd(const int32_t* nodetab, const int32_t* pairs, const float* x0, float* z_out, int64_t B,
                              int64_t N, int64_t D, int64_t hops, float alpha, int flags, void* workspace,
                              int64_t ws_bytes, lg_stream_t stream) {
    const int rc = df_check(nodetab, pairs, x0, z_out, B, N, D, hops, alpha);
    if (rc != LG_OK) return rc;
    if (flags & ~LG_F_DIFFUSE_HOPWISE) return LG_EUNSUPPORTED;
    const int64_t need = lg_diffuse_workspace_bytes(B, N, D, hops, flags, 0);
    if (need > 0 && (!workspace || ws_bytes < need)) return LG_EINVAL;
    if (B == 0) return LG_OK;
    hipStream_t s = lg_stream(stream);
    if (df_resident(N, D, flags))
        return df_launch_res<false, false>(df_slice(N, D), nodetab, pairs, x0, nullptr, z_out, B, N, D, hops, alpha, 1.f, s);
    // hop k (1-based) writes z_out when K - k is even, else the workspace: the last hop lands in
    // z_out and never reads it
    float* tmp = static_cast<float*>(workspace);
    const float* src = x0;
    for (int64_t k = 1; k <= hops; ++k) {
        float* dst = ((hops - k) % 2 == 0) ? z_out : tmp;
        df_launch_hop<false, false>(nodetab, pairs, src, x0, nullptr, dst, B, N, D, alpha, 1.f, k == 1, k == hops, s);
        src = dst;
    }
    LG_RET_IF_LAUNCH_FAILED();
    return LG_OK;
}

extern "C" int lg_diffuse_bwd(const int32_t* nodetab_t, const int32_t* pairs_t, const float* g, const float* x0,
                              float* dx0_out, int64_t B, int64_t N, int64_t D, int64_t hops, float alpha, int flags,
                              float scale_out, void* workspace, int64_t ws_bytes, lg_stream_t stream) {
    const int rc = df_check(nodetab_t, pairs_t, g, dx0_out, B, N, D, hops, alpha);
    if (rc != LG_OK) return rc;
    if (flags & ~(LG_F_DIFFUSE_HOPWISE | LG_F_MASK_OUT)) return LG_EUNSUPPORTED;
    const bool mask = (flags & LG_F_MASK_OUT) != 0;
    if (mask && (!x0 || x0 == dx0_out)) return LG_EINVAL;
    const int64_t need = lg_diffuse_workspace_bytes(B, N, D, hops, flags, 1);
    if (need > 0 && (!workspace || ws_bytes < need)) return LG_EINVAL;
    if (B == 0) return LG_OK;
    hipStream_t s = lg_stream(stream);
    if (df_resident(N, D, flags)) {
        const int cs = df_slice(N, D);
        return mask ? df_launch_res<true, true>(cs, nodetab_t, pairs_t, g, x0, dx0_out, B, N, D, hops, alpha, scale_out, s)
                    : df_launch_res<true, false>(cs, nodetab_t, pairs_t, g, nullptr, dx0_out, B, N, D, hops, alpha, 1.f, s);
    }
    float* tmp = static_cast<float*>(workspace);
    float* acc = hops >= 2 ? tmp + N * B * D : nullptr;
    const float* src = g;
    for (int64_t k = 1; k <= hops; ++k) {
        float* dst = ((hops - k) % 2 == 0) ? dx0_out : tmp;
        if (mask) df_launch_hop<true, true>(nodetab_t, pairs_t, src, x0, acc, dst, B, N, D, alpha, scale_out, k == 1, k == hops, s);
        else df_launch_hop<true, false>(nodetab_t, pairs_t, src, nullptr, acc, dst, B, N, D, alpha, 1.f, k == 1, k == hops, s);
        src = dst;
    }
    LG_RET_IF_LAUNCH_FAILED();
    return LG_OK;
}
