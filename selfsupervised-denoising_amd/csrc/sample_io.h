// sample_io.h -- what the image, tile and pool ops (image_io.hip, tile_io.hip, patch_pool.hip) share: the two sample models, byte and
// uint16, as policies their kernels are templates over; the index helpers reflect and n2v_pick (the latter also elementwise.hip's); the
// 32 x 64 patch the image and tile kernels walk.  Definitions: include/ssdn_hip.h; DESIGN.md sections 3.16 and 3.18 - 3.20.
#pragma once
#include "common.h"

static constexpr int TI = 32, TJ = 64;                         // patch: tensor axis 2 (image x), tensor axis 3 (image y)
static constexpr int IB = 256;                                 // threads of a block
static constexpr int CMAX = 3;
static_assert(TJ == 64 && IB % 64 == 0, "the plane side maps a wave's lanes to the 64 consecutive elements of one patch row");
static_assert((TJ * TI) % IB == 0 && TI % (IB / 64) == 0, "every thread takes the same number of samples and of plane elements");

// numpy's "reflect" for any pad length: index k >= 0 of an axis of n >= 1 elements continued without repeating its ends
static __device__ __forceinline__ int reflect(int k, int n) {
    if (k < n) return k;                                        // (inside the extent: most of a picture)
    if (n == 1) return 0;
    const int p = 2 * (n - 1), m = k % p;
    return m < n ? m : p - m;
}

// uniform integer over [lo, hi) without c (at least one candidate is assumed; n2v_ups.py:40-46); negative results wrap (Python indexing)
static __device__ __forceinline__ int n2v_pick(int c, int r, int size, float u) {
    const int lo = c - r < 0 ? c - r : 0, hi = c + r < size - 1 ? c + r : size - 1;
    int span = hi - lo - (c >= lo && c < hi ? 1 : 0);
    if (span < 1) span = 1;
    int k = (int)(u * (float)span);
    if (k >= span) k = span - 1;
    int v = lo + k;
    if (c >= lo && c < hi && v >= c) ++v;
    if (v < 0) v += size;
    if (v >= size) v = size - 1;
    return v;
}

static __device__ __forceinline__ float clip01(float v) {
    v = v > 0.f ? v : 0.f;                                      // (NaN and -0.0 end here)
    return v < 1.f ? v : 1.f;
}

// A sample policy is built from an op's argument struct.  T: the sample in memory; in: sample -> value; out: value -> sample, as an
// unsigned word for the LDS tile; noun, field: the words of the launchers' error texts; white_ok: the host check of what it holds.
struct ByteSample {
    typedef uint8_t T;
    static constexpr const char* noun = "byte";
    static constexpr const char* field = "bytes";
    template <class A>
    __device__ __forceinline__ explicit ByteSample(A) {}        // (by value: a reference to the kernel's arguments that nothing reads still changed k_tile_out's code)
    template <class A>
    static bool white_ok(const A&) { return true; }
    __device__ __forceinline__ float in(T s) const { return (float)s / 255.f; }          // (a true division, like to_tensor's)
    // q: np.uint8(np.clip(v, 0, 1) * 255), the reference's tensor2image: a float32 product, then truncation; NaN -> 0
    __device__ __forceinline__ unsigned out(float v) const { return (unsigned)__fmul_rn(clip01(v), 255.f); }
};

// white: the sample value that means 1.0
struct WideSample {
    typedef uint16_t T;
    static constexpr const char* noun = "sample";
    static constexpr const char* field = "count";
    unsigned white;
    float fwhite;
    template <class A>
    __device__ __forceinline__ explicit WideSample(const A& a) : white((unsigned)a.white), fwhite((float)a.white) {}
    template <class A>
    static bool white_ok(const A& a) { return a.white >= 1 && a.white <= 65535; }
    __device__ __forceinline__ float in(T s) const { return __fdiv_rn((float)min((unsigned)s, white), fwhite); }   // (a true division; a sample above white is 1.0)
    // q16: clip to [0, 1], one float32 product, round to nearest even (the product is at most 65535: exact in the conversion); NaN -> 0.
    // It rounds where q truncates: it has no reference to follow, and truncation does not survive the round trip out(in(s)) = s
    __device__ __forceinline__ unsigned out(float v) const { return (unsigned)rintf(__fmul_rn(clip01(v), fwhite)); }
};

// the length of an op's sample buffer, in samples: the byte structs call it *_bytes, the uint16 structs *_count
static __host__ __device__ __forceinline__ long long sample_count(const ssdn_image_in_args& a) { return a.src_bytes; }
static __host__ __device__ __forceinline__ long long sample_count(const ssdn_image_in16_args& a) { return a.src_count; }
static __host__ __device__ __forceinline__ long long sample_count(const ssdn_image_out_args& a) { return a.dst_bytes; }
static __host__ __device__ __forceinline__ long long sample_count(const ssdn_image_out16_args& a) { return a.dst_count; }
static __host__ __device__ __forceinline__ long long sample_count(const ssdn_tile_in_args& a) { return a.src_bytes; }
static __host__ __device__ __forceinline__ long long sample_count(const ssdn_tile_in16_args& a) { return a.src_count; }
