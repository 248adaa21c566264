// philox.h -- the library's counter-based random numbers, shared by the training patch stream (elementwise.hip: SSDN_OP_NOISE) and the
// posterior sampler (head_posterior.hip: SSDN_OP_HEAD_POSTERIOR): Philox4x32-10, the map of 32 random bits to (0, 1] and the Box-Muller
// normal.  A value is a pure function of (key, counter); the callers lay the counter out as (element, stream, offset lo, offset hi) and key
// it by the seed.  Streams: 0..4 are SSDN_OP_NOISE's (NS_* in elementwise.hip); 5 (NS_CROP in patch_pool.hip) is SSDN_OP_POOL_PATCH's crop and transform draw, which also reads stream 3 as SSDN_OP_NOISE does; PH_STREAM_POSTERIOR and above are the posterior sampler's.
#pragma once

struct Ph4 { unsigned v[4]; };
static __device__ __forceinline__ Ph4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    Ph4 o;
    o.v[0] = c0; o.v[1] = c1; o.v[2] = c2; o.v[3] = c3;
    return o;
}
static __device__ __forceinline__ float u01(unsigned x) { return (float)(x >> 8) * (1.f / 16777216.f) + (0.5f / 16777216.f); }   // (0, 1]: the top 256 words round up to 1.0
// one N(0,1) value from two random words (Box-Muller, the cosine branch)
static __device__ __forceinline__ float ph_normal(unsigned a, unsigned b) {
    return sqrtf(-2.f * __logf(u01(a))) * __cosf(6.28318530718f * u01(b));
}
// ... and both branches: two independent N(0,1) values from the same two words
static __device__ __forceinline__ void ph_normal2(unsigned a, unsigned b, float& z0, float& z1) {
    const float r = sqrtf(-2.f * __logf(u01(a))), t = 6.28318530718f * u01(b);
    z0 = r * __cosf(t);
    z1 = r * __sinf(t);
}
// first stream id of the posterior sampler: sample s draws from streams PH_STREAM_POSTERIOR + 2 s (normals) and + 2 s + 1 (the impulse
// mixture's decision); SSDN_OP_NOISE uses 0..4
#define PH_STREAM_POSTERIOR 0x80000000u
