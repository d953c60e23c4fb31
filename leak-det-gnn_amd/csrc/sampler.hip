// The datasets' per-sample decisions and the window gather on the device.
//   lg_draw_detector / lg_draw_predictor : sample idx's (scene, t, label, ...) from numpy's own stream of
//       default_rng(seed + idx) (np_rng.h), one thread per sample, the RNG calls of
//       AbruptLeakDetectorDataset.draw / NormalPredictorDataset.draw in their order
//       (models/datasets.py), into one int32[8] record per sample;
//   lg_gather_windows : one workgroup per sample copies the sample's windows out of the HBM-resident
//       scene bank and writes its label / pipe index / bucket code.
//   *_host twins run the same draw code on the CPU over host tables (tests/test_sampler_host.py).
// The draw functions below are the single statement of the sampling rules for both sides.
#include <algorithm>
#include <climits>
#include "common.h"
#include "np_rng.h"

namespace {

constexpr int kDrawThreads = 256;
constexpr int kGatherThreads = 256;
constexpr int kRec = LG_DRAW_RECORD;  // int32 words per record
constexpr int kAttempts = 10;         // datasets.py: `for _ in range(10)`

struct DetTables {
    const int32_t* leak_list;    // bank scene index of every entry of ds.leak_scene_ids
    const int32_t* noleak_list;  // ... of ds.noleak_scene_ids
    const int32_t* times;        // [n_scenes][4][2]: (start, count) of the scene's time list per bucket
    const int32_t* pipe;         // [n_scenes]: pipe index, -1 for a no-leak scene
    int32_t n_leak, n_noleak, n_scenes, no_leak_class;
    double cum[4];
};

struct PredTables {
    const int32_t* list;       // bank scene index of every entry of ds.scene_ids
    const int32_t* scene_len;  // [n_scenes]: T of the scene
    int32_t n_list, n_scenes, l_in, h;
};

__host__ __device__ __forceinline__ void put_record(int32_t* rec, int32_t scene, int32_t t, int32_t label,
                                                    int32_t pipe, int32_t bucket, int32_t attempts) {
    rec[0] = scene, rec[1] = t, rec[2] = label, rec[3] = pipe, rec[4] = bucket, rec[5] = attempts;
    rec[6] = 0, rec[7] = 0;
}

// false: no attempt found a non-empty time list (or a table entry points outside the bank); the
// record then has label -1 and nothing in it may be used as an index.
__host__ __device__ __forceinline__ bool draw_detector(const DetTables& tb, uint64_t entropy, int32_t* rec) {
    NpRng r = np_seed(entropy);
    for (int a = 1; a <= kAttempts; ++a) {
        const double u = np_random(r);
        const int b = u < tb.cum[0] ? 0 : u < tb.cum[1] ? 1 : u < tb.cum[2] ? 2 : 3;
        const int32_t scene = b == 3 ? tb.noleak_list[np_bounded(r, static_cast<uint64_t>(tb.n_noleak))]
                                     : tb.leak_list[np_bounded(r, static_cast<uint64_t>(tb.n_leak))];
        if (scene < 0 || scene >= tb.n_scenes) break;
        const int32_t start = tb.times[(scene * 4 + b) * 2], count = tb.times[(scene * 4 + b) * 2 + 1];
        if (count <= 0) continue;
        const int32_t t = start + static_cast<int32_t>(np_bounded(r, static_cast<uint64_t>(count)));
        const int32_t pipe = b == 3 ? -1 : tb.pipe[scene];
        put_record(rec, scene, t, b < 2 ? pipe : tb.no_leak_class, pipe, b, a);
        return true;
    }
    put_record(rec, -1, -1, -1, -1, -1, kAttempts);
    return false;
}

__host__ __device__ __forceinline__ bool draw_predictor(const PredTables& tb, uint64_t entropy, int32_t* rec) {
    NpRng r = np_seed(entropy);
    const int32_t scene = tb.list[np_bounded(r, static_cast<uint64_t>(tb.n_list))];
    if (scene >= 0 && scene < tb.n_scenes) {
        const int64_t count = static_cast<int64_t>(tb.scene_len[scene]) - tb.h - tb.l_in + 1;
        if (count >= 1) {
            const int32_t t = tb.l_in - 1 + static_cast<int32_t>(np_bounded(r, static_cast<uint64_t>(count)));
            put_record(rec, scene, t, 0, -1, -1, 1);
            return true;
        }
    }
    put_record(rec, -1, -1, -1, -1, -1, 1);
    return false;
}

__global__ void __launch_bounds__(kDrawThreads)
k_draw_detector(DetTables tb, uint64_t seed, int64_t i0, int64_t n, int32_t* __restrict__ records,
                unsigned* __restrict__ err) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kDrawThreads + threadIdx.x;
    if (i >= n) return;
    int32_t rec[kRec];
    const bool ok = draw_detector(tb, seed + static_cast<uint64_t>(i0 + i), rec);
#pragma unroll
    for (int k = 0; k < kRec; ++k) records[i * kRec + k] = rec[k];
    if (!ok) atomicAdd(err, 1u);
}

__global__ void __launch_bounds__(kDrawThreads)
k_draw_predictor(PredTables tb, uint64_t seed, int64_t i0, int64_t n, int32_t* __restrict__ records,
                 unsigned* __restrict__ err) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kDrawThreads + threadIdx.x;
    if (i >= n) return;
    int32_t rec[kRec];
    const bool ok = draw_predictor(tb, seed + static_cast<uint64_t>(i0 + i), rec);
#pragma unroll
    for (int k = 0; k < kRec; ++k) records[i * kRec + k] = rec[k];
    if (!ok) atomicAdd(err, 1u);
}

struct GatherSeg {
    const float* src;  // bank tensor [n_scenes][T_max][C]; nullptr: segment unused
    float* dst;        // batch tensor [n][len][C]
    int32_t C, off, len;
};
struct GatherArgs {
    const int32_t* records;
    int64_t n;
    int32_t n_scenes, T_max;
    GatherSeg seg[3];
    int64_t* label;
    int64_t* pipe_index;
    int32_t* bucket_code;
    unsigned* err;  // err[1]: records of a decided sample that point outside the bank
};

__global__ void __launch_bounds__(kGatherThreads) k_gather_windows(GatherArgs a) {
    const int64_t s = blockIdx.x;  // one workgroup per sample: everything below is uniform in it
    const int32_t* rec = a.records + s * kRec;
    const int32_t scene = rec[0], t = rec[1], label = rec[2];
    bool ok = label >= 0;
    if (ok) {  // a decided sample's windows must lie inside the bank before any address is formed
        bool in = scene >= 0 && scene < a.n_scenes;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (a.seg[k].src) {
                const int64_t first = static_cast<int64_t>(t) + a.seg[k].off;
                in = in && first >= 0 && first + a.seg[k].len <= a.T_max;
            }
        if (!in) {
            ok = false;
            if (threadIdx.x == 0) atomicAdd(a.err + 1, 1u);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const GatherSeg g = a.seg[k];
        if (!g.src) continue;
        const int total = g.len * g.C;
        float* dst = g.dst + s * total;
        if (ok) {
            const float* src = g.src + (static_cast<int64_t>(scene) * a.T_max + t + g.off) * g.C;
            for (int i = threadIdx.x; i < total; i += kGatherThreads) dst[i] = src[i];
        } else {
            for (int i = threadIdx.x; i < total; i += kGatherThreads) dst[i] = 0.f;
        }
    }
    if (threadIdx.x == 0) {
        if (a.label) a.label[s] = ok ? label : -1;
        if (a.pipe_index) a.pipe_index[s] = ok ? rec[3] : -1;
        if (a.bucket_code) a.bucket_code[s] = ok ? rec[4] : -1;
    }
}

bool det_args_ok(int64_t i0, int64_t n, const void* leak_list, int64_t n_leak, const void* noleak_list,
                 int64_t n_noleak, const void* times, const void* pipe, int64_t n_scenes, const double* cum_host,
                 int64_t no_leak_class, const void* records, const void* err) {
    if (i0 < 0 || n < 0 || n > LG_DRAW_MAX_SAMPLES) return false;
    if (n_leak < 1 || n_noleak < 1 || n_scenes < 1 || n_leak > INT32_MAX || n_noleak > INT32_MAX) return false;
    if (n_scenes > INT32_MAX / 8 || no_leak_class < 0 || no_leak_class > INT32_MAX) return false;
    if (!leak_list || !noleak_list || !times || !pipe || !cum_host || !err) return false;
    for (int k = 0; k < 4; ++k)
        if (!(cum_host[k] >= 0.0 && cum_host[k] <= 1.0 + 1e-6) || (k && cum_host[k] < cum_host[k - 1])) return false;
    return n == 0 || records;
}

DetTables det_tables(const int32_t* leak_list, int64_t n_leak, const int32_t* noleak_list, int64_t n_noleak,
                     const int32_t* times, const int32_t* pipe, int64_t n_scenes, const double* cum_host,
                     int64_t no_leak_class) {
    DetTables tb{};
    tb.leak_list = leak_list, tb.noleak_list = noleak_list, tb.times = times, tb.pipe = pipe;
    tb.n_leak = static_cast<int32_t>(n_leak), tb.n_noleak = static_cast<int32_t>(n_noleak);
    tb.n_scenes = static_cast<int32_t>(n_scenes), tb.no_leak_class = static_cast<int32_t>(no_leak_class);
    for (int k = 0; k < 4; ++k) tb.cum[k] = cum_host[k];
    return tb;
}

bool pred_args_ok(int64_t i0, int64_t n, const void* list, int64_t n_list, const void* scene_len, int64_t n_scenes,
                  int64_t l_in, int64_t h, const void* records, const void* err) {
    if (i0 < 0 || n < 0 || n > LG_DRAW_MAX_SAMPLES) return false;
    if (n_list < 1 || n_list > INT32_MAX || n_scenes < 1 || n_scenes > INT32_MAX) return false;
    if (l_in < 1 || h < 0 || l_in > (1 << 24) || h > (1 << 24)) return false;
    if (!list || !scene_len || !err) return false;
    return n == 0 || records;
}

}  // namespace

extern "C" int lg_draw_detector(uint64_t seed, int64_t i0, int64_t n, const int32_t* leak_list, int64_t n_leak,
                                const int32_t* noleak_list, int64_t n_noleak, const int32_t* times,
                                const int32_t* pipe, int64_t n_scenes, const double* cum_host, int64_t no_leak_class,
                                int32_t* records, uint32_t* err, lg_stream_t stream) {
    if (!det_args_ok(i0, n, leak_list, n_leak, noleak_list, n_noleak, times, pipe, n_scenes, cum_host, no_leak_class,
                     records, err))
        return LG_EINVAL;
    if (n == 0) return LG_OK;
    const DetTables tb = det_tables(leak_list, n_leak, noleak_list, n_noleak, times, pipe, n_scenes, cum_host,
                                    no_leak_class);
    const int grid = static_cast<int>((n + kDrawThreads - 1) / kDrawThreads);
    lg_launch(k_draw_detector, grid, kDrawThreads, 0, lg_stream(stream), tb, seed, i0, n, records, err);
    LG_RET_IF_LAUNCH_FAILED();
    return LG_OK;
}

extern "C" int lg_draw_detector_host(uint64_t seed, int64_t i0, int64_t n, const int32_t* leak_list_host,
                                     int64_t n_leak, const int32_t* noleak_list_host, int64_t n_noleak,
                                     const int32_t* times_host, const int32_t* pipe_host, int64_t n_scenes,
                                     const double* cum_host, int64_t no_leak_class, int32_t* records_host,
                                     uint32_t* err_host) {
    if (!det_args_ok(i0, n, leak_list_host, n_leak, noleak_list_host, n_noleak, times_host, pipe_host, n_scenes,
                     cum_host, no_leak_class, records_host, err_host))
        return LG_EINVAL;
    const DetTables tb = det_tables(leak_list_host, n_leak, noleak_list_host, n_noleak, times_host, pipe_host,
                                    n_scenes, cum_host, no_leak_class);
    for (int64_t i = 0; i < n; ++i)
        if (!draw_detector(tb, seed + static_cast<uint64_t>(i0 + i), records_host + i * kRec)) err_host[0] += 1;
    return LG_OK;
}

extern "C" int lg_draw_predictor(uint64_t seed, int64_t i0, int64_t n, const int32_t* scene_list, int64_t n_list,
                                 const int32_t* scene_len, int64_t n_scenes, int64_t l_in, int64_t h,
                                 int32_t* records, uint32_t* err, lg_stream_t stream) {
    if (!pred_args_ok(i0, n, scene_list, n_list, scene_len, n_scenes, l_in, h, records, err)) return LG_EINVAL;
    if (n == 0) return LG_OK;
    const PredTables tb{scene_list, scene_len, static_cast<int32_t>(n_list), static_cast<int32_t>(n_scenes),
                        static_cast<int32_t>(l_in), static_cast<int32_t>(h)};
    const int grid = static_cast<int>((n + kDrawThreads - 1) / kDrawThreads);
    lg_launch(k_draw_predictor, grid, kDrawThreads, 0, lg_stream(stream), tb, seed, i0, n, records, err);
    LG_RET_IF_LAUNCH_FAILED();
    return LG_OK;
}

extern "C" int lg_draw_predictor_host(uint64_t seed, int64_t i0, int64_t n, const int32_t* scene_list_host,
                                      int64_t n_list, const int32_t* scene_len_host, int64_t n_scenes, int64_t l_in,
                                      int64_t h, int32_t* records_host, uint32_t* err_host) {
    if (!pred_args_ok(i0, n, scene_list_host, n_list, scene_len_host, n_scenes, l_in, h, records_host, err_host))
        return LG_EINVAL;
    const PredTables tb{scene_list_host, scene_len_host, static_cast<int32_t>(n_list),
                        static_cast<int32_t>(n_scenes), static_cast<int32_t>(l_in), static_cast<int32_t>(h)};
    for (int64_t i = 0; i < n; ++i)
        if (!draw_predictor(tb, seed + static_cast<uint64_t>(i0 + i), records_host + i * kRec)) err_host[0] += 1;
    return LG_OK;
}

extern "C" int lg_np_stream_host(uint64_t seed, const int32_t* ops_host, const int64_t* low_host,
                                 const uint64_t* count_host, int64_t n, double* out_f_host, int64_t* out_i_host) {
    if (n < 0 || (n > 0 && (!ops_host || !low_host || !count_host || !out_f_host || !out_i_host))) return LG_EINVAL;
    for (int64_t k = 0; k < n; ++k) {  // the whole script is checked before any draw
        if (ops_host[k] != LG_NP_RANDOM && ops_host[k] != LG_NP_BOUNDED) return LG_EINVAL;
        if (ops_host[k] == LG_NP_BOUNDED && !np_count_ok(count_host[k])) return LG_EINVAL;
    }
    NpRng r = np_seed(seed);
    for (int64_t k = 0; k < n; ++k) {
        out_f_host[k] = 0.0;
        out_i_host[k] = 0;
        if (ops_host[k] == LG_NP_RANDOM)
            out_f_host[k] = np_random(r);
        else
            out_i_host[k] = low_host[k] + static_cast<int64_t>(np_bounded(r, count_host[k]));
    }
    return LG_OK;
}

extern "C" int lg_gather_windows(const int32_t* records, int64_t n, int64_t n_scenes, int64_t T_max,
                                 const float* src0, int64_t C0, int64_t off0, int64_t len0, float* dst0,
                                 const float* src1, int64_t C1, int64_t off1, int64_t len1, float* dst1,
                                 const float* src2, int64_t C2, int64_t off2, int64_t len2, float* dst2,
                                 int64_t* label, int64_t* pipe_index, int32_t* bucket_code, uint32_t* err,
                                 lg_stream_t stream) {
    if (n < 0 || n > INT32_MAX || n_scenes < 1 || n_scenes > INT32_MAX || T_max < 1 || T_max > INT32_MAX || !err)
        return LG_EINVAL;
    const float* src[3] = {src0, src1, src2};
    float* dst[3] = {dst0, dst1, dst2};
    const int64_t C[3] = {C0, C1, C2}, off[3] = {off0, off1, off2}, len[3] = {len0, len1, len2};
    GatherArgs a{};
    for (int k = 0; k < 3; ++k) {
        if (!src[k]) continue;
        if (C[k] < 1 || len[k] < 1 || len[k] > T_max || off[k] < -T_max || off[k] > T_max) return LG_EINVAL;
        if (C[k] * len[k] > (1 << 24)) return LG_EINVAL;  // a sample's segment is indexed with 32 bits
        if (n > 0 && !dst[k]) return LG_EINVAL;
        a.seg[k] = GatherSeg{src[k], dst[k], static_cast<int32_t>(C[k]), static_cast<int32_t>(off[k]),
                             static_cast<int32_t>(len[k])};
    }
    if (n == 0) return LG_OK;
    if (!records) return LG_EINVAL;
    a.records = records;
    a.n = n;
    a.n_scenes = static_cast<int32_t>(n_scenes), a.T_max = static_cast<int32_t>(T_max);
    a.label = label, a.pipe_index = pipe_index, a.bucket_code = bucket_code;
    a.err = err;
    lg_launch(k_gather_windows, static_cast<int>(n), kGatherThreads, 0, lg_stream(stream), a);
    LG_RET_IF_LAUNCH_FAILED();
    return LG_OK;
}
