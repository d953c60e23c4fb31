// GRU layers at H = 128 (NormalPredictorGRU, reference models/predictor.py:84-111) on exact
// fp32 MFMA (v_mfma_f32_16x16x4_f32), PyTorch gate order and formulas (see gru.hip).
//
// Forward.  One workgroup = 16 sequences x 8 waves; wave w owns hidden units [16w, 16w + 16)
// of ALL THREE gates, so r, z, n and the new h of a (unit, sequence) meet in one lane and
// the only exchange per step is the new h through LDS (double-buffered, one barrier per
// step).  The wave keeps its 48 rows of W_hh as A fragments in registers (96 VGPRs) and, in
// the dense form with I <= 48 (the predictor's first layer, I = S + 9), its rows of W_ih too
// (K zero-padded to 48, 36 VGPRs).  Wider inputs stream W_ih from memory every step (both sets
// of fragments do not fit 256 VGPRs), 16-byte loads when I % 4 == 0 (the upper layers, I =
// 128), 128 columns of x staged at a time.  The x rows of step t + 1
// are loaded while step t computes.  The K index is permuted as in gru.hip (fk), so a lane
// reads its B operands from LDS four at a time.
// In the window form the input gates W_ih x + b_ih are read in place from gi [B][T][3H]:
// sequence q = k * B + b (shift-major) reads row (b, k + t) at step t, so the l_det windows of
// a segment share one (l_pred + l_det)-row product and are never unfolded.
//
// Backward.  A recurrence kernel carries only the dh chain: per step it forms the gate
// gradients of its lane's (unit, sequence), posts dG_h to LDS, and dh_{t-1} = z dh_t +
// W_hh^T dG_h on W_hh^T fragments held in registers (96 VGPRs).  It writes dG
// [steps][Nseq][4][H] = (dG_r, dG_z, dG_in, dG_hn) for a pass of steps into the workspace;
// three GEMM kernels then take dW_ih = dG_i^T x_eff and dW_hh = dG_h^T h_{t-1} (with the bias
// sums) as per-row-block partials that a later pass adds to in place, and dx = dG_i W_ih
// times the dropout mask and scale.  The partials are reduced in fixed order (reduce.h), so
// every gradient is deterministic.  All offsets are 64-bit.
#include <algorithm>
#include "common.h"
#include "gru128.h"
#include "reduce.h"

namespace {

constexpr int H = 128, G3 = 3 * H, G4 = 4 * H;
constexpr int TS = 16;       // sequences per workgroup
constexpr int NTH = 512;     // 8 waves
constexpr int HS = H + 4;    // LDS row stride of the h / x tiles (16-byte rows, conflict-free reads)
constexpr int DS = G3 + 4;   // LDS row stride of the backward's dG tile

__device__ __forceinline__ f32x4 mfma(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ int fk(int ks, int q) { return 16 * (ks >> 2) + 4 * q + (ks & 3); }
// gru.hip's gate nonlinearities (hardware exp2 / rcp, a few ulp)
__device__ __forceinline__ float sigm(float x) {
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504088896341f * x));
}
__device__ __forceinline__ float gru_tanh(float x) {
    const float ax = fabsf(x);
    const float t = __builtin_amdgcn_exp2f(-2.88539008177792682f * ax);
    const float big = (1.0f - t) * __builtin_amdgcn_rcpf(1.0f + t);
    const float x2 = x * x;
    const float small = ax * fmaf(x2, fmaf(x2, 0.133333333333f, -0.333333333333f), 1.0f);
    return copysignf(ax < 0.0625f ? small : big, x);
}
__device__ __forceinline__ f32x4 zero4() { return f32x4{0.f, 0.f, 0.f, 0.f}; }
__device__ __forceinline__ float drop1(const LgGru128Drop& d, uint32_t key, float v, uint64_t idx) {
    return d.on ? lg_dropout(v, d.p, d.scale, key, idx) : v;
}

// KI > 0: k-steps of W_ih held in registers (I <= 4 KI); KI < 0: W_ih streamed from memory (any I);
// KI == 0: window form, the input gates come from gi.
template <int KI, bool SAVE>
__global__ void __launch_bounds__(NTH)
k_gru128_fwd(const float* __restrict__ x, const float* __restrict__ Wih, const float* __restrict__ Whh,
             const float* __restrict__ bih, const float* __restrict__ bhh, const float* __restrict__ gi,
             float* __restrict__ hs, float* __restrict__ gates, float* __restrict__ hlast, uint32_t Nseq, int L, int I,
             uint32_t B, uint32_t T, LgGru128Drop dr) {
    constexpr bool WIN = KI == 0;
    constexpr int KR = KI > 0 ? KI : 1;
    __shared__ __attribute__((aligned(16))) float hl[2][TS * HS];
    __shared__ __attribute__((aligned(16))) float xs[2][TS * HS];  // x_t, columns [0, 128)
    __shared__ __attribute__((aligned(16))) float xe[TS * HS];     // x_t, a later 128-column chunk
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, j = lane & 15, q = lane >> 4;
    const uint32_t seq0 = blockIdx.x * TS, seq = seq0 + j;
    const bool valid = seq < Nseq;
    const int u4 = 16 * w + 4 * q;  // the lane's four units
    const uint32_t key = (!WIN && dr.on) ? lg_dropout_key_dev(dr.seed, dr.salt) : 0u;

    float ah[32][3], ai[KR][3];
#pragma unroll
    for (int ks = 0; ks < 32; ++ks)
#pragma unroll
        for (int g = 0; g < 3; ++g) ah[ks][g] = Whh[static_cast<size_t>(g * H + 16 * w + j) * H + fk(ks, q)];
    if constexpr (KI > 0) {
#pragma unroll
        for (int ks = 0; ks < KI; ++ks) {
            const int c = fk(ks, q);
#pragma unroll
            for (int g = 0; g < 3; ++g) ai[ks][g] = c < I ? Wih[static_cast<size_t>(g * H + 16 * w + j) * I + c] : 0.f;
        }
    }
    f32x4 br, bz, bn, bhn;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int u = u4 + reg;
        br[reg] = bhh[u] + (WIN ? 0.f : bih[u]);
        bz[reg] = bhh[H + u] + (WIN ? 0.f : bih[H + u]);
        bn[reg] = WIN ? 0.f : bih[2 * H + u];
        bhn[reg] = bhh[2 * H + u];
    }
    for (int e = threadIdx.x; e < TS * HS; e += NTH) hl[0][e] = 0.f;  // h_{-1} = 0

    // x staging: element e = threadIdx.x + 512 i of the [16][128] tile, row e >> 7, column e & 127
    float xr[4];
    auto load_x = [&](int t, int c0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = threadIdx.x + NTH * i, row = e >> 7, col = c0 + (e & 127);
            xr[i] = 0.f;
            if (seq0 + row < Nseq && col < I) {
                const uint64_t idx = (static_cast<uint64_t>(t) * Nseq + seq0 + row) * static_cast<uint64_t>(I) + col;
                xr[i] = drop1(dr, key, x[idx], idx);
            }
        }
    };
    auto store_x = [&](float* dst) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = threadIdx.x + NTH * i;
            dst[(e >> 7) * HS + (e & 127)] = xr[i];
        }
    };
    // window form: the lane's gi row at step 0; step t + 1's input gates are loaded during step t
    const float* girow = nullptr;
    f32x4 gr_ = zero4(), gz_ = zero4(), gn_ = zero4();
    auto load_gi = [&](int t) {
        if (valid) {
            const float* g = girow + static_cast<size_t>(t) * G3;
            gr_ = ld4(g);
            gz_ = ld4(g + H);
            gn_ = ld4(g + 2 * H);
        }
    };
    if constexpr (WIN) {
        if (valid) {
            const uint32_t k = seq / B, b = seq - k * B;
            girow = gi + (static_cast<size_t>(b) * T + k) * G3 + u4;
        }
        load_gi(0);
    } else {
        load_x(0, 0);
        store_x(xs[0]);
    }
    __syncthreads();

    f32x4 hcur = zero4();
    for (int t = 0; t < L; ++t) {
        const int cur = t & 1, nxt = cur ^ 1;
        f32x4 ar = br, az = bz, an = bn, ahn = bhn;
        if constexpr (WIN) {
            ar += gr_;
            az += gz_;
            an += gn_;
            if (t + 1 < L) load_gi(t + 1);
        } else {
            if (t + 1 < L) load_x(t + 1, 0);
        }
        const float* hrow = &hl[cur][j * HS + 4 * q];
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
            const f32x4 hv = ld4(hrow + 16 * kk);
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                ar = mfma(ah[4 * kk + p][0], hv[p], ar);
                az = mfma(ah[4 * kk + p][1], hv[p], az);
                ahn = mfma(ah[4 * kk + p][2], hv[p], ahn);
            }
        }
        if constexpr (KI > 0) {  // I <= 4 KI: W_ih in registers
            const float* xrow = &xs[cur][j * HS + 4 * q];
#pragma unroll
            for (int kk = 0; kk < KI / 4; ++kk) {
                const f32x4 xv = ld4(xrow + 16 * kk);
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    ar = mfma(ai[4 * kk + p][0], xv[p], ar);
                    az = mfma(ai[4 * kk + p][1], xv[p], az);
                    an = mfma(ai[4 * kk + p][2], xv[p], an);
                }
            }
        } else if constexpr (KI < 0) {  // wider inputs: W_ih streamed from memory, 128 columns at a time
            float keep[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) keep[i] = xr[i];
            const bool vec = (I & 3) == 0;
            const float* wr = Wih + static_cast<size_t>(16 * w + j) * I;
            const size_t gs = static_cast<size_t>(H) * I;  // gate stride
            for (int c0 = 0; c0 < I; c0 += H) {
                const float* xrow = &xs[cur][j * HS + 4 * q];
                if (c0 > 0) {  // columns past 128 are staged here, one chunk at a time
                    __syncthreads();  // the previous chunk's reads of xe
                    load_x(t, c0);
                    store_x(xe);
                    __syncthreads();
                    xrow = &xe[j * HS + 4 * q];
                }
                const int nkk = (min(I - c0, H) + 15) / 16;
                for (int kk = 0; kk < nkk; ++kk) {
                    const int c = c0 + 16 * kk + 4 * q;
                    const f32x4 xv = ld4(xrow + 16 * kk);
                    f32x4 wa = zero4(), wb = zero4(), wc = zero4();
                    if (vec) {
                        if (c < I) {
                            wa = ld4(wr + c);
                            wb = ld4(wr + gs + c);
                            wc = ld4(wr + 2 * gs + c);
                        }
                    } else {
#pragma unroll
                        for (int p = 0; p < 4; ++p) {
                            if (c + p < I) {
                                wa[p] = wr[c + p];
                                wb[p] = wr[gs + c + p];
                                wc[p] = wr[2 * gs + c + p];
                            }
                        }
                    }
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        ar = mfma(wa[p], xv[p], ar);
                        az = mfma(wb[p], xv[p], az);
                        an = mfma(wc[p], xv[p], an);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) xr[i] = keep[i];
        }
        f32x4 r, z, n;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            r[reg] = sigm(ar[reg]);
            z[reg] = sigm(az[reg]);
            n[reg] = gru_tanh(an[reg] + r[reg] * ahn[reg]);
            hcur[reg] = (1.f - z[reg]) * n[reg] + z[reg] * hcur[reg];
        }
        if (!valid) hcur = zero4();
        st4(&hl[nxt][j * HS + u4], hcur);
        if constexpr (!WIN) {
            if (t + 1 < L) store_x(xs[nxt]);
        }
        if (valid) {
            const size_t row = static_cast<size_t>(t) * Nseq + seq;
            if (hs) st4(hs + row * H + u4, hcur);
            if constexpr (SAVE) {
                float* gr = gates + row * G4 + u4;
                st4(gr, r);
                st4(gr + H, z);
                st4(gr + 2 * H, n);
                st4(gr + 3 * H, ahn);
            }
            if (hlast && t == L - 1) st4(hlast + static_cast<size_t>(seq) * H + u4, hcur);
        }
        __syncthreads();
    }
}

// The dh chain over steps [t0, t1), t descending.  init: 0 = dh starts at zero, 1 = at dhc (the
// carry the previous pass left); dhL (or NULL) is added at t = L - 1.  Leaves the carry in dhc.
__global__ void __launch_bounds__(NTH)
k_gru128_bwd_rec(const float* __restrict__ Whh, const float* __restrict__ hs, const float* __restrict__ gates,
                 const float* __restrict__ dhS, const float* __restrict__ dhL, float* __restrict__ dhc,
                 float* __restrict__ dG, uint32_t Nseq, int t0, int t1, int L, int init) {
    __shared__ __attribute__((aligned(16))) float dgl[2][TS * DS];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, j = lane & 15, q = lane >> 4;
    const uint32_t seq = blockIdx.x * TS + j;
    const bool valid = seq < Nseq;
    const int u4 = 16 * w + 4 * q;

    float at[96];  // W_hh^T: A[unit 16w + j][gate row fk(ks, q)]
#pragma unroll
    for (int ks = 0; ks < 96; ++ks) at[ks] = Whh[static_cast<size_t>(fk(ks, q)) * H + 16 * w + j];

    f32x4 dh = zero4();
    if (valid && init) dh = ld4(dhc + static_cast<size_t>(seq) * H + u4);
    int buf = 0;
    for (int t = t1 - 1; t >= t0; --t) {
        f32x4 r = zero4(), z = zero4(), n = zero4(), hn = zero4(), hp = zero4();
        if (valid) {
            const size_t row = static_cast<size_t>(t) * Nseq + seq;
            const float* gr = gates + row * G4 + u4;
            r = ld4(gr);
            z = ld4(gr + H);
            n = ld4(gr + 2 * H);
            hn = ld4(gr + 3 * H);
            if (t > 0) hp = ld4(hs + (row - Nseq) * H + u4);
            if (dhS) dh += ld4(dhS + row * H + u4);
            if (dhL && t == L - 1) dh += ld4(dhL + static_cast<size_t>(seq) * H + u4);
        }
        f32x4 dgr, dgz, dgn, dghn;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const float dn = dh[reg] * (1.f - z[reg]) * (1.f - n[reg] * n[reg]);
            dgn[reg] = dn;
            dghn[reg] = dn * r[reg];
            dgr[reg] = dn * hn[reg] * r[reg] * (1.f - r[reg]);
            dgz[reg] = dh[reg] * (hp[reg] - n[reg]) * z[reg] * (1.f - z[reg]);
        }
        float* dl = &dgl[buf][j * DS + u4];
        st4(dl, dgr);
        st4(dl + H, dgz);
        st4(dl + 2 * H, dghn);
        if (valid) {
            float* go = dG + (static_cast<size_t>(t - t0) * Nseq + seq) * G4 + u4;
            st4(go, dgr);
            st4(go + H, dgz);
            st4(go + 2 * H, dgn);
            st4(go + 3 * H, dghn);
        }
        __syncthreads();
        f32x4 acc = dh * z;
        const float* drow = &dgl[buf][j * DS + 4 * q];
#pragma unroll
        for (int kk = 0; kk < 24; ++kk) {
            const f32x4 v = ld4(drow + 16 * kk);
#pragma unroll
            for (int p = 0; p < 4; ++p) acc = mfma(at[4 * kk + p], v[p], acc);
        }
        dh = acc;
        buf ^= 1;
    }
    if (valid) st4(dhc + static_cast<size_t>(seq) * H + u4, dh);
}

// Partial weight gradients of one pass: block (rb, mt, nt) sums its rows of
//   out[m][n] = sum_r dG[r][col(m)] * Bm[r][n]
// for the 64 gate rows m = 64 mt .. and the 128 columns n = 128 nt .., into slab row rb (added to
// what is there when accum).  hh == 0: Bm = x_eff (ldb = N = I, dropout on read), gate slots
// (r, z, in); hh == 1: Bm = h_{t-1} (the h_seq row one step earlier, zero at t = 0), gate slots
// (r, z, hn).  The column sums of dG (the bias gradient) ride along in the nt == 0 blocks.
constexpr int AS = 80, BS = 144;  // LDS row strides (conflict-free fragment reads)
__global__ void __launch_bounds__(256)
k_gru128_dw(const float* __restrict__ dG, const float* __restrict__ Bm, float* __restrict__ slab, int64_t slab_len,
            int64_t off_w, int64_t off_b, int64_t R, int64_t rpb, int64_t row0, int64_t shift, int N, int hh,
            int accum, LgGru128Drop dr) {
    __shared__ __attribute__((aligned(16))) float ag[16 * AS];
    __shared__ __attribute__((aligned(16))) float bg[16 * BS];
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, j = lane & 15, q = lane >> 4;
    const int mt = blockIdx.y, n0 = 128 * blockIdx.z;
    const int cbase = (hh && mt >= 4) ? G3 + 64 * (mt - 4) : 64 * mt;
    const int64_t rb0 = static_cast<int64_t>(blockIdx.x) * rpb;
    const int64_t rbeg = rb0 < R ? rb0 : R, rend = rbeg + rpb < R ? rbeg + rpb : R;
    const uint32_t key = dr.on ? lg_dropout_key_dev(dr.seed, dr.salt) : 0u;
    f32x4 acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = zero4();
    float dbs = 0.f;
    for (int64_t r0 = rbeg; r0 < rend; r0 += 16) {
        {
            const int row = threadIdx.x >> 4, c4 = (threadIdx.x & 15) * 4;
            f32x4 v = zero4();
            if (r0 + row < rend) v = ld4(dG + static_cast<size_t>(r0 + row) * G4 + cbase + c4);
            st4(&ag[row * AS + c4], v);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int e = threadIdx.x + 256 * i, row = e >> 7, col = e & 127;
            const int64_t grow = row0 + r0 + row;
            float v = 0.f;
            if (r0 + row < rend && n0 + col < N && grow >= shift) {
                const uint64_t idx = static_cast<uint64_t>(grow - shift) * static_cast<uint64_t>(N) + n0 + col;
                v = drop1(dr, key, Bm[idx], idx);
            }
            bg[row * BS + col] = v;
        }
        __syncthreads();
        if (blockIdx.z == 0 && threadIdx.x < 64) {
#pragma unroll
            for (int row = 0; row < 16; ++row) dbs += ag[row * AS + threadIdx.x];
        }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const float a = ag[(4 * ks + q) * AS + 16 * wv + j];
#pragma unroll
            for (int nt = 0; nt < 8; ++nt) acc[nt] = mfma(a, bg[(4 * ks + q) * BS + 16 * nt + j], acc[nt]);
        }
        __syncthreads();
    }
    float* out = slab + static_cast<size_t>(blockIdx.x) * slab_len;
#pragma unroll
    for (int nt = 0; nt < 8; ++nt) {
        const int n = n0 + 16 * nt + j;
        if (n < N) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                float* o = out + off_w + static_cast<size_t>(64 * mt + 16 * wv + 4 * q + reg) * N + n;
                *o = accum ? *o + acc[nt][reg] : acc[nt][reg];
            }
        }
    }
    if (blockIdx.z == 0 && threadIdx.x < 64) {
        float* o = out + off_b + 64 * mt + threadIdx.x;
        *o = accum ? *o + dbs : dbs;
    }
}

// dx[r][i] = (sum_c dG_i[r][c] W_ih[c][i]) * mask * scale for the R rows of a pass; block =
// 64 rows x 128 columns, W_ih staged 32 gate rows at a time.
__global__ void __launch_bounds__(256)
k_gru128_dx(const float* __restrict__ dG, const float* __restrict__ Wih, float* __restrict__ dx, int64_t R,
            int64_t row0, int I, LgGru128Drop dr) {
    __shared__ __attribute__((aligned(16))) float wl[32 * BS];
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63, j = lane & 15, q = lane >> 4;
    const int n0 = 128 * blockIdx.y;
    const int64_t rbase = static_cast<int64_t>(blockIdx.x) * 64 + 16 * wv;
    const int64_t arow = rbase + j;  // the lane's A row
    const uint32_t key = dr.on ? lg_dropout_key_dev(dr.seed, dr.salt) : 0u;
    f32x4 acc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = zero4();
    for (int c0 = 0; c0 < G3; c0 += 32) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int e = threadIdx.x + 256 * i, cr = e >> 7, col = e & 127;
            wl[cr * BS + col] = n0 + col < I ? Wih[static_cast<size_t>(c0 + cr) * I + n0 + col] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            f32x4 a = zero4();
            if (arow < R) a = ld4(dG + static_cast<size_t>(arow) * G4 + c0 + 16 * kk + 4 * q);
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const float* wrow = &wl[(16 * kk + 4 * q + p) * BS + j];
#pragma unroll
                for (int nt = 0; nt < 8; ++nt) acc[nt] = mfma(a[p], wrow[16 * nt], acc[nt]);
            }
        }
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
        const int64_t r = rbase + 4 * q + reg;
        if (r >= R) continue;
#pragma unroll
        for (int nt = 0; nt < 8; ++nt) {
            const int n = n0 + 16 * nt + j;
            if (n < I) {
                const uint64_t idx = static_cast<uint64_t>(row0 + r) * static_cast<uint64_t>(I) + n;
                dx[idx] = drop1(dr, key, acc[nt][reg], idx);
            }
        }
    }
}

inline int64_t slab_len128(int64_t I) { return G3 * (H + I) + 2 * G3; }
inline int64_t slab_rows128(int64_t Nseq) { return std::max<int64_t>(1, std::min<int64_t>(32, (Nseq + 7) / 8)); }
constexpr int64_t kPassBudget = int64_t{64} << 20;  // dG bytes of one pass the workspace query plans for
inline int64_t fixed_floats128(int64_t Nseq, int64_t I) { return slab_rows128(Nseq) * slab_len128(I) + Nseq * H; }

}  // namespace

int lg_gru128_fwd(const float* x, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                  float* h_seq, float* gates, float* h_last, int64_t Nseq, int64_t L, int64_t I,
                  const LgGru128Drop& dr, hipStream_t s) {
    const unsigned grid = static_cast<unsigned>((Nseq + TS - 1) / TS);
    const uint32_t n = static_cast<uint32_t>(Nseq);
#define LG_GRU128_FWD(KI, SV)                                                                                    \
    lg_launch(k_gru128_fwd<KI, SV>, grid, NTH, 0, s, x, w_ih, w_hh, b_ih, b_hh, nullptr, h_seq, gates, h_last, n, \
              static_cast<int>(L), static_cast<int>(I), 1u, 1u, dr)
    if (I <= 48) { if (gates) LG_GRU128_FWD(12, true); else LG_GRU128_FWD(12, false); }
    else { if (gates) LG_GRU128_FWD(-1, true); else LG_GRU128_FWD(-1, false); }
#undef LG_GRU128_FWD
    LG_RET_IF_LAUNCH_FAILED();
    return LG_OK;
}

int lg_gru128_win_fwd(const float* gi, const float* w_hh, const float* b_hh, float* h_seq, float* h_last, int64_t B,
                      int64_t T, int64_t l_pred, int64_t n_win, hipStream_t s) {
    const int64_t Nseq = n_win * B;
    const unsigned grid = static_cast<unsigned>((Nseq + TS - 1) / TS);
    lg_launch(k_gru128_fwd<0, false>, grid, NTH, 0, s, nullptr, nullptr, w_hh, nullptr, b_hh, gi, h_seq, nullptr, h_last,
              static_cast<uint32_t>(Nseq), static_cast<int>(l_pred), 0, static_cast<uint32_t>(B),
              static_cast<uint32_t>(T), LgGru128Drop{0, 0.f, 1.f, 0, 0});
    LG_RET_IF_LAUNCH_FAILED();
    return LG_OK;
}

int64_t lg_gru128_bwd_ws_bytes(int64_t Nseq, int64_t I) {
    const int64_t step = std::max<int64_t>(1, Nseq) * G4 * static_cast<int64_t>(sizeof(float));
    const int64_t steps = std::max<int64_t>(1, std::min<int64_t>(1024, kPassBudget / step));
    return fixed_floats128(Nseq, I) * static_cast<int64_t>(sizeof(float)) + steps * step;
}

int lg_gru128_bwd(const float* x, const float* w_ih, const float* w_hh, const float* h_seq, const float* gates,
                  const float* dh_seq, const float* dh_last, float* dx, float* dw_ih, float* dw_hh, float* db_ih,
                  float* db_hh, int64_t Nseq, int64_t L, int64_t I, const LgGru128Drop& dr, void* workspace,
                  int64_t ws_bytes, hipStream_t s) {
    const int64_t len = slab_len128(I), nb = slab_rows128(Nseq);
    const int64_t fixed = fixed_floats128(Nseq, I);
    const int64_t step = std::max<int64_t>(1, Nseq) * G4;  // dG floats per step
    const int64_t have = ws_bytes / static_cast<int64_t>(sizeof(float)) - fixed;
    if (have < step) return LG_EINVAL;
    const int64_t Tc = std::min<int64_t>(L, have / step);
    float* slab = static_cast<float*>(workspace);
    float* dhc = slab + nb * len;
    float* dG = dhc + Nseq * H;
    const int64_t offWhh = 0, offWih = static_cast<int64_t>(G3) * H, offBih = offWih + G3 * I, offBhh = offBih + G3;
    if (Nseq == 0) {
        if (hipMemsetAsync(slab, 0, sizeof(float) * len, s) != hipSuccess) return LG_EHIP;
    }
    const LgGru128Drop nodrop{0, 0.f, 1.f, 0, 0};
    const unsigned seqblocks = static_cast<unsigned>((Nseq + TS - 1) / TS);
    for (int64_t t1 = L; t1 > 0 && Nseq > 0; t1 -= Tc) {
        const int64_t t0 = std::max<int64_t>(0, t1 - Tc);
        const int first = t1 == L;
        lg_launch(k_gru128_bwd_rec, seqblocks, NTH, 0, s, w_hh, h_seq, gates, dh_seq, dh_last, dhc, dG,
                  static_cast<uint32_t>(Nseq), static_cast<int>(t0), static_cast<int>(t1), static_cast<int>(L),
                  first ? 0 : 1);
        LG_RET_IF_LAUNCH_FAILED();
        const int64_t R = (t1 - t0) * Nseq, row0 = t0 * Nseq;
        const int64_t rpb = ((R + nb - 1) / nb + 15) / 16 * 16;
        lg_launch(k_gru128_dw, dim3(static_cast<unsigned>(nb), 6, static_cast<unsigned>((I + 127) / 128)), 256, 0, s, dG,
                  x, slab, len, offWih, offBih, R, rpb, row0, int64_t{0}, static_cast<int>(I), 0, first ? 0 : 1, dr);
        LG_RET_IF_LAUNCH_FAILED();
        lg_launch(k_gru128_dw, dim3(static_cast<unsigned>(nb), 6, 1), 256, 0, s, dG, h_seq, slab, len, offWhh, offBhh, R,
                  rpb, row0, Nseq, static_cast<int>(H), 1, first ? 0 : 1, nodrop);
        LG_RET_IF_LAUNCH_FAILED();
        if (dx) {
            lg_launch(k_gru128_dx, dim3(static_cast<unsigned>((R + 63) / 64), static_cast<unsigned>((I + 127) / 128)), 256,
                      0, s, dG, w_ih, dx, R, row0, static_cast<int>(I), dr);
            LG_RET_IF_LAUNCH_FAILED();
        }
    }
    const LgSlabSeg segs[4] = {{offWhh, static_cast<int64_t>(G3) * H, dw_hh}, {offWih, G3 * I, dw_ih},
                               {offBih, G3, db_ih}, {offBhh, G3, db_hh}};
    return lg_launch_slab_reduce_multi(slab, static_cast<int>(nb), len, segs, 4, nullptr, nullptr, s);
}
