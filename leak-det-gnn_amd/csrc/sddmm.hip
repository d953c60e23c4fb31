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
