// numpy's default_rng(seed) stream, restated as host + device code: SeedSequence(entropy) ->
// generate_state(4, uint64) -> PCG64 (XSL-RR 128/64) -> Generator.random() / .integers() /
// scalar .choice().  The datasets draw every sample from np.random.default_rng(seed + idx)
// (models/datasets.py), so a sampler that replays this stream reproduces them bit for bit.
// The installed numpy is the oracle (tests/test_sampler_host.py); the constants are numpy's
// (_seed_sequence.pyx, pcg64.h, distributions.c).  Plain C++: the one 128-bit step is a
// 64 x 64 -> 128 multiply written with a high-half helper.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NP_HD __host__ __device__ __forceinline__
#else
#define NP_HD inline
#endif

NP_HD uint64_t np_mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return static_cast<uint64_t>((static_cast<unsigned __int128>(a) * b) >> 64);
#endif
}

struct NpRng {
    uint64_t hi, lo;          // PCG64 state
    uint64_t inc_hi, inc_lo;  // PCG64 increment (odd)
    uint32_t half;            // the buffered high half of the last next64 taken by next32
    bool has_half;
};

NP_HD void np_step(NpRng& r) {
    constexpr uint64_t kMulHi = 0x2360ED051FC65DA4ull, kMulLo = 0x4385DF649FCCF645ull;
    const uint64_t lo = r.lo * kMulLo;
    const uint64_t hi = np_mulhi64(r.lo, kMulLo) + r.hi * kMulLo + r.lo * kMulHi;
    r.lo = lo + r.inc_lo;
    r.hi = hi + r.inc_hi + (r.lo < lo ? 1u : 0u);
}

// SeedSequence's hashmix: `hc` is carried from call to call.
NP_HD uint32_t np_hashmix(uint32_t v, uint32_t& hc) {
    v ^= hc;
    hc *= 0x931e8875u;
    v *= hc;
    v ^= v >> 16;
    return v;
}
NP_HD uint32_t np_mix(uint32_t x, uint32_t y) {
    uint32_t r = 0xca01f9ddu * x - 0x4973f715u * y;
    r ^= r >> 16;
    return r;
}

// default_rng(entropy), entropy in [0, 2^64): one 32-bit word below 2^32, else two, padded to the
// pool's four with zeros (a zero word hashes like an absent one, so no word count is needed).
NP_HD NpRng np_seed(uint64_t entropy) {
    uint32_t pool[4] = {static_cast<uint32_t>(entropy), static_cast<uint32_t>(entropy >> 32), 0u, 0u};
    uint32_t hc = 0x43b0d7e5u;
    for (int i = 0; i < 4; ++i) pool[i] = np_hashmix(pool[i], hc);
    for (int s = 0; s < 4; ++s)
        for (int d = 0; d < 4; ++d)
            if (s != d) pool[d] = np_mix(pool[d], np_hashmix(pool[s], hc));
    // generate_state(4, uint64): eight words, word 2k the low half of value k
    uint32_t w[8];
    uint32_t hb = 0x8b51f9ddu;
    for (int i = 0; i < 8; ++i) {
        uint32_t v = pool[i & 3];
        v ^= hb;
        hb *= 0x58f38dedu;
        v *= hb;
        v ^= v >> 16;
        w[i] = v;
    }
    const uint64_t v0 = (static_cast<uint64_t>(w[1]) << 32) | w[0], v1 = (static_cast<uint64_t>(w[3]) << 32) | w[2];
    const uint64_t v2 = (static_cast<uint64_t>(w[5]) << 32) | w[4], v3 = (static_cast<uint64_t>(w[7]) << 32) | w[6];
    NpRng r;
    r.inc_hi = (v2 << 1) | (v3 >> 63);  // inc = (initseq << 1) | 1, initseq = v2 : v3
    r.inc_lo = (v3 << 1) | 1u;
    r.hi = r.lo = 0;
    r.half = 0;
    r.has_half = false;
    np_step(r);
    const uint64_t lo = r.lo + v1;      // state += initstate, initstate = v0 : v1
    r.hi = r.hi + v0 + (lo < r.lo ? 1u : 0u);
    r.lo = lo;
    np_step(r);
    return r;
}

NP_HD uint64_t np_next64(NpRng& r) {
    np_step(r);
    const uint64_t x = r.hi ^ r.lo;
    const unsigned rot = static_cast<unsigned>(r.hi >> 58);  // state >> 122
    return (x >> rot) | (x << ((64u - rot) & 63u));
}

NP_HD uint32_t np_next32(NpRng& r) {
    if (r.has_half) {
        r.has_half = false;
        return r.half;
    }
    const uint64_t v = np_next64(r);
    r.has_half = true;
    r.half = static_cast<uint32_t>(v >> 32);
    return static_cast<uint32_t>(v);
}

// Generator.random(): leaves the buffered half alone
NP_HD double np_random(NpRng& r) { return static_cast<double>(np_next64(r) >> 11) * (1.0 / 9007199254740992.0); }

// Generator.integers(low, low + count) for 1 <= count <= 2^32, which is also scalar
// Generator.choice over `count` items (low = 0): returns the offset from low.  count = 1 draws
// nothing; count = 2^32 is one next32; else Lemire's rejection on 32 bits.  The caller refuses
// any other count (np_count_ok) before calling.
NP_HD bool np_count_ok(uint64_t count) { return count >= 1 && count <= (uint64_t{1} << 32); }
NP_HD uint32_t np_bounded(NpRng& r, uint64_t count) {
    const uint32_t rng = static_cast<uint32_t>(count - 1);
    if (rng == 0) return 0;
    if (rng == 0xFFFFFFFFu) return np_next32(r);
    const uint32_t ex = rng + 1;
    uint64_t m = static_cast<uint64_t>(np_next32(r)) * ex;
    uint32_t left = static_cast<uint32_t>(m);
    if (left < ex) {
        const uint32_t th = (0xFFFFFFFFu - rng) % ex;
        while (left < th) {
            m = static_cast<uint64_t>(np_next32(r)) * ex;
            left = static_cast<uint32_t>(m);
        }
    }
    return static_cast<uint32_t>(m >> 32);
}
