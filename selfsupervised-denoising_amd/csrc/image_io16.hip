// image_io16.hip -- SSDN_OP_IMAGE_IN16 / SSDN_OP_IMAGE_OUT16: whole 16-bit images of differing sizes into and out of the engine as uint16
// samples (gfx950).  No planned list holds them.  Definition and contract: include/ssdn_hip.h; the sample model, kernel shape and
// measurements: DESIGN.md section 3.20.  The kernels are image_io.hip's with a sample of two bytes: the same 32 x 64 tile, the same LDS tile
// of odd pitch holding fp32 (in) or unsigned words (out), so the bank behaviour is the sibling's.  Counts, offsets and indices are in
// SAMPLES; the byte kernels and their file stay as they are.
// k_image_in16:  samples -> min(s, white) / white -> LDS (a row per (x, c)) -> fp32 planes.
// k_image_out16: fp32 planes -> clip, * white, round to nearest even -> LDS -> samples.
#include "common.h"

static constexpr int TI = 32, TJ = 64;                         // tile: tensor axis 2 (image x), tensor axis 3 (image y)
static constexpr int IB = 256;                                 // threads of a block
static constexpr int CMAX = 3;
static_assert(TJ == 64 && IB % 64 == 0, "the plane side maps a wave's lanes to the 64 consecutive elements of one tile row");
static_assert((TJ * TI) % IB == 0 && TI % (IB / 64) == 0, "every thread takes the same number of samples and of plane elements");

// a sample's extent, clamped to the tensor (ext is device memory: nothing on the host has seen it)
static __device__ __forceinline__ void image_extent(const int32_t* ext, int b, int H, int W, int& e1, int& e2) {
    e1 = min(max(ext[2 * b], 0), H);
    e2 = min(max(ext[2 * b + 1], 0), W);
}

// numpy's "reflect" for any pad length: index k >= 0 of an axis of n >= 1 elements continued without repeating its ends
static __device__ __forceinline__ int reflect(int k, int n) {
    if (k < n) return k;
    if (n == 1) return 0;
    const int p = 2 * (n - 1), m = k % p;
    return m < n ? m : p - m;
}

// sample `idx` of the image at sample `off` lies inside the buffer of `count` samples (off is device memory too)
static __device__ __forceinline__ bool image_inside(long long off, long long idx, long long count) {
    return off >= 0 && off < count && idx < count - off;
}

template <int C>
__global__ __launch_bounds__(IB) void k_image_in16(ssdn_image_in16_args a) {
    __shared__ float tile[TI * CMAX][TJ + 1];
    const int b = blockIdx.z, i0 = blockIdx.y * TI, j0 = blockIdx.x * TJ;
    int e1, e2;
    image_extent(a.ext, b, a.H, a.W, e1, e2);
    const long long off = a.offs[b];
    const bool any = e1 > 0 && e2 > 0;                          // (block-uniform: a sample without an extent becomes zeros)
    const unsigned white = (unsigned)a.white;
    const float fwhite = (float)a.white;
    // samples: consecutive lanes take consecutive (x, c) of one image row; every load of the thread is issued before the first is used
    constexpr int NB = TJ * TI * C / IB;
    unsigned short raw[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        const int t = threadIdx.x + u * IB;
        const int jj = t / (TI * C), xb = t - jj * (TI * C);
        const int ii = xb / C, c = xb - ii * C;
        raw[u] = 0;
        if (any && i0 + ii < a.H && j0 + jj < a.W) {
            const long long idx = ((long long)reflect(j0 + jj, e2) * e1 + reflect(i0 + ii, e1)) * C + c;
            if (image_inside(off, idx, a.src_count)) raw[u] = a.src[off + idx];
        }
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        const int t = threadIdx.x + u * IB;
        const int jj = t / (TI * C), xb = t - jj * (TI * C);
        tile[xb][jj] = __fdiv_rn((float)min((unsigned)raw[u], white), fwhite);      // (a true division; a sample above white is 1.0)
    }
    __syncthreads();
    // planes: a wave stores the 64 consecutive elements of one (c, i) row
    const int lane = threadIdx.x & 63, j = j0 + lane;
#pragma unroll
    for (int u = 0; u < TI * C / (IB / 64); ++u) {
        const int r = (threadIdx.x >> 6) + u * (IB / 64);
        const int c = r / TI, ii = r - c * TI, i = i0 + ii;
        if (i < a.H && j < a.W) a.dst[(((long long)b * C + c) * a.H + i) * a.W + j] = tile[ii * C + c][lane];
    }
}

// q16: clip to [0, 1], one float32 product, round to nearest even (the product is at most 65535: exact in the conversion); NaN -> 0
static __device__ __forceinline__ unsigned quantise16(float v, float fwhite) {
    v = v > 0.f ? v : 0.f;                                      // (NaN and -0.0 end here)
    v = v < 1.f ? v : 1.f;
    return (unsigned)rintf(__fmul_rn(v, fwhite));
}

template <int C>
__global__ __launch_bounds__(IB) void k_image_out16(ssdn_image_out16_args a) {
    __shared__ unsigned tile[TI * CMAX][TJ + 1];
    const int b = blockIdx.z, i0 = blockIdx.y * TI, j0 = blockIdx.x * TJ;
    int e1, e2;
    image_extent(a.ext, b, a.H, a.W, e1, e2);
    if (i0 >= e1 || j0 >= e2) return;                           // (block-uniform: the tile lies outside the extent)
    const long long off = a.offs[b];
    const float fwhite = (float)a.white;
    const int lane = threadIdx.x & 63, j = j0 + lane;
    // planes: every load of the thread is issued before the first is used
    constexpr int NP = TI * C / (IB / 64);
    float v[NP];
#pragma unroll
    for (int u = 0; u < NP; ++u) {
        const int r = (threadIdx.x >> 6) + u * (IB / 64);
        const int c = r / TI, ii = r - c * TI, i = i0 + ii;
        v[u] = (i < e1 && j < e2) ? a.x[(((long long)b * C + c) * a.H + i) * a.W + j] : 0.f;      // (e1 <= H, e2 <= W)
    }
#pragma unroll
    for (int u = 0; u < NP; ++u) {
        const int r = (threadIdx.x >> 6) + u * (IB / 64);
        const int c = r / TI, ii = r - c * TI;
        tile[ii * C + c][lane] = quantise16(v[u], fwhite);
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < TJ * TI * C / IB; ++u) {
        const int t = threadIdx.x + u * IB;
        const int jj = t / (TI * C), xb = t - jj * (TI * C);
        const int ii = xb / C, c = xb - ii * C;
        if (i0 + ii < e1 && j0 + jj < e2) {
            const long long idx = ((long long)(j0 + jj) * e1 + (i0 + ii)) * C + c;
            if (image_inside(off, idx, a.dst_count)) a.dst[off + idx] = (uint16_t)tile[xb][jj];
        }
    }
}

// the checks both ops share; `op` is the prefix of the error text
static int image_io16_check(const char* op, const void* samples, long long count, const void* offs, const void* ext, const void* planes,
                            int B, int C, int H, int W, int white) {
    if (!samples || !offs || !ext || !planes) return ssdn_set_error("%s: the sample buffer, offs, ext and the tensor must be given", op);
    if (C != 1 && C != 3) return ssdn_set_error("%s: C must be 1 or 3", op);
    if (B < 1 || H < 1 || W < 1) return ssdn_set_error("%s: B, H and W must be at least 1", op);
    if (count < 0) return ssdn_set_error("%s: the sample count must not be negative", op);
    if (white < 1 || white > 65535) return ssdn_set_error("%s: white must lie in [1, 65535]", op);
    if (B > 65535 || (H + TI - 1) / TI > 65535) return ssdn_set_error("%s: B and the tile rows must be at most 65535", op);
    return 0;
}

int launch_image_in16(const ssdn_image_in16_args* a, hipStream_t s) {
    if (int rc = image_io16_check("image_in16", a->src, a->src_count, a->offs, a->ext, a->dst, a->B, a->C, a->H, a->W, a->white)) return rc;
    const dim3 grid((unsigned)((a->W + TJ - 1) / TJ), (unsigned)((a->H + TI - 1) / TI), (unsigned)a->B);
    if (a->C == 1) hipLaunchKernelGGL(k_image_in16<1>, grid, dim3(IB), 0, s, *a);
    else hipLaunchKernelGGL(k_image_in16<3>, grid, dim3(IB), 0, s, *a);
    return 0;
}

int launch_image_out16(const ssdn_image_out16_args* a, hipStream_t s) {
    if (int rc = image_io16_check("image_out16", a->dst, a->dst_count, a->offs, a->ext, a->x, a->B, a->C, a->H, a->W, a->white)) return rc;
    const dim3 grid((unsigned)((a->W + TJ - 1) / TJ), (unsigned)((a->H + TI - 1) / TI), (unsigned)a->B);
    if (a->C == 1) hipLaunchKernelGGL(k_image_out16<1>, grid, dim3(IB), 0, s, *a);
    else hipLaunchKernelGGL(k_image_out16<3>, grid, dim3(IB), 0, s, *a);
    return 0;
}
