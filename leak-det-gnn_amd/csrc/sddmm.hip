// Sampled dense-dense product over a CSR (lg_sddmm_cols): out[k] = a[row(k)] . b[col[k]] for
// every slot k.  The gradient of a propagate with respect to its coefficients (edge weights):
// GCNConv's dL/dw[k] = dy[n] . (x W^T)[col k], lg_spmm_cols' dL/dw[k] = dy[n] . x[col k].
//
// One wave walks one row at a time.  Its 64 lanes form 64 / LPE groups of LPE lanes; a group
// takes one CSR entry, its lanes the columns (four consecutive floats per lane and 16-byte
// loads when C, both strides and both bases allow, else one float).  The row's `a` values stay
// in the lanes' registers for all of the row's entries; every pass gathers two entries per
// group, so 2 * 64 / LPE neighbour rows are in flight per wave (8 at C = 64).  A group's dot
// product is its lanes' partial sums added by an xor butterfly of fixed shape, so a result
// never depends on scheduling; no atomics.
#include <algorithm>

#include "common.h"

namespace {

template <int V>
struct Unit;
template <>
struct Unit<4> {
    using T = f32x4;
    static __device__ __forceinline__ T load(const float* p) { return ld4(p); }
    static __device__ __forceinline__ T zero() { return f32x4{0.f, 0.f, 0.f, 0.f}; }
    static __device__ __forceinline__ float fma(T x, T y, float s) {
#pragma unroll
        for (int i = 0; i < 4; ++i) s = fmaf(x[i], y[i], s);
        return s;
    }
};
template <>
struct Unit<1> {
    using T = float;
    static __device__ __forceinline__ T load(const float* p) { return *p; }
    static __device__ __forceinline__ T zero() { return 0.f; }
    static __device__ __forceinline__ float fma(T x, T y, float s) { return fmaf(x, y, s); }
};

// V: floats per lane unit (4 or 1); LPE: lanes per entry (a power of two <= 64); R: units of a
// row a lane holds in registers (columns past LPE * R * V, only at LPE == 64, are re-read per
// entry); IX: uint32_t when every element offset N * ld fits 32 bits, else int64_t.
template <int V, int LPE, int R, typename IX>
__global__ void __launch_bounds__(256) k_sddmm_cols(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                    const float* __restrict__ a, int64_t lda,
                                                    const float* __restrict__ b, int64_t ldb, float* __restrict__ out,
                                                    int64_t N, int64_t C) {
    using U = Unit<V>;
    using T = typename U::T;
    constexpr int EPW = 64 / LPE;  // entries per wave and gather
    const int lane = threadIdx.x & 63;
    const int g = lane / LPE, l = lane % LPE;
    const int units = static_cast<int>(C / V);
    const int64_t wave = static_cast<int64_t>(blockIdx.x) * (blockDim.x >> 6) +
                         __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    const int64_t nwaves = static_cast<int64_t>(gridDim.x) * (blockDim.x >> 6);
    const IX la = static_cast<IX>(lda), lb = static_cast<IX>(ldb);
    for (int64_t n = wave; n < N; n += nwaves) {
        const int e0 = rowptr[n], e1 = rowptr[n + 1];
        const float* arow = a + static_cast<IX>(n) * la;
        T av[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int u = l + r * LPE;
            av[r] = u < units ? U::load(arow + u * V) : U::zero();
        }
        for (int base = e0; base < e1; base += 2 * EPW) {
            const int k0 = base + g, k1 = k0 + EPW;
            const bool v0 = k0 < e1, v1 = k1 < e1;
            int c0 = v0 ? col[k0] : 0, c1 = v1 ? col[k1] : 0;
            if (c0 < 0 || c0 >= N) c0 = 0;  // a malformed CSR never reads out of range
            if (c1 < 0 || c1 >= N) c1 = 0;
            const float* b0 = b + static_cast<IX>(c0) * lb;
            const float* b1 = b + static_cast<IX>(c1) * lb;
            T x0[R], x1[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {  // all gathers of the pass before the first use
                const int u = l + r * LPE;
                x0[r] = (v0 && u < units) ? U::load(b0 + u * V) : U::zero();
                x1[r] = (v1 && u < units) ? U::load(b1 + u * V) : U::zero();
            }
            float s0 = 0.f, s1 = 0.f;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                s0 = U::fma(av[r], x0[r], s0);
                s1 = U::fma(av[r], x1[r], s1);
            }
            if constexpr (LPE == 64 && R > 1) {  // columns past the registers
                for (int u = l + R * LPE; u < units; u += LPE) {
                    const T y = U::load(arow + u * V);
                    if (v0) s0 = U::fma(y, U::load(b0 + u * V), s0);
                    if (v1) s1 = U::fma(y, U::load(b1 + u * V), s1);
                }
            }
#pragma unroll
            for (int off = LPE / 2; off >= 1; off >>= 1) {  // stays inside the group of LPE lanes
                s0 += __shfl_xor(s0, off, 64);
                s1 += __shfl_xor(s1, off, 64);
            }
            if (l == 0) {
                if (v0) out[k0] = s0;
                if (v1) out[k1] = s1;
            }
        }
    }
}

template <int V, int LPE, int R>
void launch_sddmm(bool i32, unsigned grid, hipStream_t s, const int32_t* rowptr, const int32_t* col, const float* a,
                  int64_t lda, const float* b, int64_t ldb, float* out, int64_t N, int64_t C) {
    if (i32) lg_launch(k_sddmm_cols<V, LPE, R, uint32_t>, grid, 256, 0, s, rowptr, col, a, lda, b, ldb, out, N, C);
    else lg_launch(k_sddmm_cols<V, LPE, R, int64_t>, grid, 256, 0, s, rowptr, col, a, lda, b, ldb, out, N, C);
}

template <int V>
void dispatch_sddmm(int64_t units, bool i32, unsigned grid, hipStream_t s, const int32_t* rowptr, const int32_t* col,
                    const float* a, int64_t lda, const float* b, int64_t ldb, float* out, int64_t N, int64_t C) {
    if (units <= 4) launch_sddmm<V, 4, 1>(i32, grid, s, rowptr, col, a, lda, b, ldb, out, N, C);
    else if (units <= 8) launch_sddmm<V, 8, 1>(i32, grid, s, rowptr, col, a, lda, b, ldb, out, N, C);
    else if (units <= 16) launch_sddmm<V, 16, 1>(i32, grid, s, rowptr, col, a, lda, b, ldb, out, N, C);
    else if (units <= 32) launch_sddmm<V, 32, 1>(i32, grid, s, rowptr, col, a, lda, b, ldb, out, N, C);
    else if (units <= 64) launch_sddmm<V, 64, 1>(i32, grid, s, rowptr, col, a, lda, b, ldb, out, N, C);
    else launch_sddmm<V, 64, 4>(i32, grid, s, rowptr, col, a, lda, b, ldb, out, N, C);
}

// ---------------------------------------------------------------------------- lg_sddmm_nm
// dL/dw of one node-major GCN layer (include/leakgnn.h): G[k] = sum_b da[n][b] . x[col k][b] with
// da = dz W formed on chip.  A tile is one node x 16 windows x D, one wave per tile, the waves
// spread over (node, window tile) so that 661 nodes still fill the machine.  Every global
// access of a tile is the trunk kernels' flat block: lane l, unit j holds the four floats at
// (j * 64 + l) * 4 of the contiguous 16 x D block, i.e. row j * RPP + l / LPR, channels
// 4 (l % LPR) .. + 3 — also the layout of the mask words (bit 4 j + i of lane l).
//   1. dz = dy (* scale * [y > 0] or the mask bit under LG_F_MASK_IN) goes to the wave's LDS tile
//      (rows padded by 4 floats: the four rows a pass reads sit in different banks);
//   2. da = dz W in exact fp32 FMA with W staged once per workgroup: lane (l, j) needs row
//      j * RPP + l / LPR of dz against columns 4 (l % LPR) .. + 3 of W, so da comes out in the
//      flat layout and needs no second trip through LDS.  (16 x D x D flops per tile against
//      (2 + deg) x 16 x D x 4 bytes of loads: the transform is not what the kernel waits for,
//      and fp32 FMA keeps da exact where a split-bf16 MFMA would add its 1e-7.)
//   3. per CSR slot of the node, two at a time: the neighbour's 16 x D block in the same flat
//      layout (one coalesced 16-byte load per lane and unit; rows past B are not read), a dot
//      product per lane, a fixed-shape xor butterfly over the wave, one partial per (tile, slot).
// k_sddmm_nm_reduce then adds a slot's partials in ascending tile order in fp64 and writes 0
// to the slots past rowptr[N].  No atomics; 32-bit element offsets (N * B * D * 4 < 2^31).
constexpr int kSddmmNmWaves = 4;

__device__ __forceinline__ void wave_sync_sd() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float dot4(f32x4 a, f32x4 b, float s) {
#pragma unroll
    for (int i = 0; i < 4; ++i) s = fmaf(a[i], b[i], s);
    return s;
}

template <int D>
__global__ void __launch_bounds__(64 * kSddmmNmWaves)
    k_sddmm_nm(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const float* __restrict__ dy,
               const float* __restrict__ y, const uint16_t* __restrict__ ymask, const float* __restrict__ W,
               const float* __restrict__ x, float* __restrict__ part, int B, int N, int T, int cap, int mask_in,
               float scale) {
    constexpr int NJ = D / 16;    // 16-byte units per lane and tile
    constexpr int LPR = D / 4;    // lanes per row
    constexpr int RPP = 64 / LPR; // rows per unit
    constexpr int LD = D + 4;     // padded row of the dz tile
    __shared__ __attribute__((aligned(16))) float sW[D * D];
    __shared__ __attribute__((aligned(16))) float sZ[kSddmmNmWaves][16 * LD];
    for (int i = threadIdx.x; i < D * D / 4; i += 64 * kSddmmNmWaves) st4(sW + 4 * i, ld4(W + 4 * i));
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
    const int r0 = lane / LPR, c0 = (lane % LPR) * 4;
    float* z = sZ[wv];
    const int ntiles = N * T;  // < 2^27: N * B * D * 4 < 2^31 and T <= (B + 15) / 16
    for (int tile = blockIdx.x * kSddmmNmWaves + wv; tile < ntiles; tile += gridDim.x * kSddmmNmWaves) {
        const int n = tile / T, t = tile - n * T;
        const uint32_t own = (static_cast<uint32_t>(n) * B + t * 16) * D;  // the tile's own block of dy / y
        const uint32_t word = mask_in && ymask ? ymask[(static_cast<uint32_t>(n) * T + t) * 64 + lane] : 0u;
        bool live[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            live[j] = t * 16 + j * RPP + r0 < B;  // a ragged last tile: rows past B are never read
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (live[j]) {
                const uint32_t e = own + (j * 64 + lane) * 4;
                v = ld4(dy + e);
                if (mask_in) {
                    if (ymask) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) v[i] = (word >> (4 * j + i)) & 1u ? v[i] * scale : 0.f;
                    } else {
                        const f32x4 yv = ld4(y + e);
#pragma unroll
                        for (int i = 0; i < 4; ++i) v[i] = yv[i] > 0.f ? v[i] * scale : 0.f;
                    }
                }
            }
            st4(z + (j * RPP + r0) * LD + c0, v);
        }
        wave_sync_sd();
        f32x4 da[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) da[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
        for (int o = 0; o < D; o += 4) {
            f32x4 wr[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) wr[i] = ld4(sW + (o + i) * D + c0);
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const f32x4 zv = ld4(z + (j * RPP + r0) * LD + o);
#pragma unroll
                for (int i = 0; i < 4; ++i) da[j] += zv[i] * wr[i];
            }
        }
        wave_sync_sd();  // the next tile's stores wait for these reads
        int e0 = rowptr[n], e1 = rowptr[n + 1];
        if (e0 < 0 || e1 > cap || e0 > e1) e0 = e1 = 0;  // a malformed CSR never writes out of range
        float* prow = part + static_cast<size_t>(t) * cap;
#pragma unroll 1
        for (int k = e0; k < e1; k += 2) {
            const bool two = k + 1 < e1;
            int ca = col[k], cb = two ? col[k + 1] : 0;
            if (ca < 0 || ca >= N) ca = 0;  // nor reads out of range
            if (cb < 0 || cb >= N) cb = 0;
            const float* xa = x + (static_cast<uint32_t>(ca) * B + t * 16) * D + lane * 4;
            const float* xb = x + (static_cast<uint32_t>(cb) * B + t * 16) * D + lane * 4;
            f32x4 va[NJ], vb[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {  // both blocks in flight before the first use
                va[j] = live[j] ? ld4(xa + j * 256) : f32x4{0.f, 0.f, 0.f, 0.f};
                vb[j] = (live[j] && two) ? ld4(xb + j * 256) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
            float sa = 0.f, sb = 0.f;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                sa = dot4(da[j], va[j], sa);
                sb = dot4(da[j], vb[j], sb);
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                sa += __shfl_xor(sa, off, 64);
                sb += __shfl_xor(sb, off, 64);
            }
            if (lane == 0) {
                prow[k] = sa;
                if (two) prow[k + 1] = sb;
            }
        }
    }
}

__global__ void __launch_bounds__(256) k_sddmm_nm_reduce(const float* __restrict__ part,
                                                         const int32_t* __restrict__ rowptr, float* __restrict__ G,
                                                         int T, int cap, int N) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= cap) return;
    int nnz = rowptr[N];
    nnz = nnz < 0 ? 0 : (nnz > cap ? cap : nnz);
    double acc = 0.0;
    if (k < nnz)
        for (int t = 0; t < T; ++t) acc += static_cast<double>(part[static_cast<size_t>(t) * cap + k]);
    G[k] = static_cast<float>(acc);
}

}  // namespace

extern "C" int lg_sddmm_cols(const int32_t* rowptr, const int32_t* col, const float* a, int64_t lda, const float* b,
                             int64_t ldb, float* out, int64_t N, int64_t C, lg_stream_t stream) {
    if (N < 0 || C < 0 || lda < C || ldb < C) return LG_EINVAL;
    if (N == 0 || C == 0) return LG_OK;
    if (!rowptr || !col || !a || !b || !out) return LG_EINVAL;
    if (N > INT32_MAX / 2 || std::max(lda, ldb) > (int64_t{1} << 62) / N) return LG_EINVAL;  // N * ld < 2^62
    hipStream_t s = lg_stream(stream);
    const bool vec = C % 4 == 0 && lda % 4 == 0 && ldb % 4 == 0 && reinterpret_cast<uintptr_t>(a) % 16 == 0 &&
                     reinterpret_cast<uintptr_t>(b) % 16 == 0;
    const bool i32 = N * std::max(lda, ldb) < (int64_t{1} << 32);
    // one wave per row, four waves per block; past 8 blocks per CU the waves stride over rows
    const unsigned grid = static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>((N + 3) / 4, 8LL * lg_num_cus())));
    if (vec) dispatch_sddmm<4>(C / 4, i32, grid, s, rowptr, col, a, lda, b, ldb, out, N, C);
    else dispatch_sddmm<1>(C, i32, grid, s, rowptr, col, a, lda, b, ldb, out, N, C);
    LG_RET_IF_LAUNCH_FAILED();
    return LG_OK;
}

extern "C" int64_t lg_sddmm_nm_workspace_bytes(int64_t B, int64_t nnz_cap) {
    if (B < 1 || nnz_cap < 0) return 0;
    return ((B + 15) / 16) * nnz_cap * static_cast<int64_t>(sizeof(float));
}

extern "C" int lg_sddmm_nm(const int32_t* rowptr, const int32_t* col, const float* dy, const float* y,
                           const uint16_t* ymask, const float* W, const float* x, float* G, int64_t B, int64_t N,
                           int64_t D, int64_t nnz_cap, int flags, float scale, void* workspace, int64_t ws_bytes,
                           lg_stream_t stream) {
    if (B < 1 || N < 0 || nnz_cap < 0) return LG_EINVAL;
    if (D != 32 && D != 64) return LG_EUNSUPPORTED;
    if (flags & ~LG_F_MASK_IN) return LG_EUNSUPPORTED;
    if (N * B * D * 4 > 0x7FFFF000LL) return LG_EUNSUPPORTED;  // 32-bit element offsets, as the trunk kernels
    const int64_t T = (B + 15) / 16;
    if (T * nnz_cap > INT32_MAX) return LG_EUNSUPPORTED;
    if (nnz_cap == 0) return LG_OK;
    if (!rowptr || !G) return LG_EINVAL;
    if (ws_bytes < lg_sddmm_nm_workspace_bytes(B, nnz_cap) || !workspace) return LG_EINVAL;
    const bool mask_in = (flags & LG_F_MASK_IN) != 0;
    hipStream_t s = lg_stream(stream);
    float* part = static_cast<float*>(workspace);
    if (N > 0) {
        if (!col || !dy || !W || !x || (mask_in && !y && !ymask)) return LG_EINVAL;
        for (const void* p : {static_cast<const void*>(dy), static_cast<const void*>(y), static_cast<const void*>(W),
                              static_cast<const void*>(x), static_cast<const void*>(part)})
            if (reinterpret_cast<uintptr_t>(p) % 16 != 0) return LG_EINVAL;
        const int64_t ntiles = N * T;
        const unsigned grid = static_cast<unsigned>(
            std::max<int64_t>(1, std::min<int64_t>((ntiles + kSddmmNmWaves - 1) / kSddmmNmWaves, 4LL * lg_num_cus())));
        const int Bi = static_cast<int>(B), Ni = static_cast<int>(N), Ti = static_cast<int>(T);
        const int capi = static_cast<int>(nnz_cap);
        if (D == 64)
            lg_launch(k_sddmm_nm<64>, grid, 64 * kSddmmNmWaves, 0, s, rowptr, col, dy, y, ymask, W, x, part, Bi, Ni, Ti,
                      capi, static_cast<int>(mask_in), scale);
        else
            lg_launch(k_sddmm_nm<32>, grid, 64 * kSddmmNmWaves, 0, s, rowptr, col, dy, y, ymask, W, x, part, Bi, Ni, Ti,
                      capi, static_cast<int>(mask_in), scale);
        LG_RET_IF_LAUNCH_FAILED();
    }
    lg_launch(k_sddmm_nm_reduce, static_cast<unsigned>((nnz_cap + 255) / 256), 256, 0, s, part, rowptr, G,
              static_cast<int>(T), static_cast<int>(nnz_cap), static_cast<int>(N));
    LG_RET_IF_LAUNCH_FAILED();
    return LG_OK;
}
