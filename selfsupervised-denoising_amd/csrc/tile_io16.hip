// tile_io16.hip -- SSDN_OP_TILE_IN16 / SSDN_OP_TILE_OUT16: one 16-bit image of any size into fixed-size overlapping tiles and the tiles'
// results back into one uint16 image, blended across the overlaps (gfx950).  No planned list holds them.  Definition and contract:
// include/ssdn_hip.h; the sample model, kernel shape and measurements: DESIGN.md section 3.20.
// The kernels are tile_io.hip's with a sample of two bytes: the same 32 x 64 patch, the same LDS tile of odd pitch holding fp32 (in) or
// unsigned words (out), the same tiling arithmetic and the same blend.  TILE_OUT16 has no mode: the fp32 std map goes through
// SSDN_OP_TILE_OUT mode 1.  Counts and indices are in SAMPLES; the byte kernels and their file stay as they are.
// The blend's difference, product and sum are rounded one by one, so contraction is off for the whole file (see lerp).
#pragma clang fp contract(off)
#include "common.h"

static constexpr int TI = 32, TJ = 64;                         // patch: along x (tensor axis 2), along y (tensor axis 3)
static constexpr int IB = 256;                                 // threads of a block
static constexpr int CMAX = 3;
static_assert(TJ == 64 && IB % 64 == 0, "the tile side maps a wave's lanes to 64 consecutive elements of tensor axis 3");
static_assert((TJ * TI) % IB == 0 && TI % (IB / 64) == 0, "every thread takes the same number of image and of tile elements");

// numpy's "reflect" for any pad length (SSDN_OP_IMAGE_IN's r): index k >= 0 of an axis of n >= 1 elements
static __device__ __forceinline__ int reflect(int k, int n) {
    if (k < n) return k;
    if (n == 1) return 0;
    const int p = 2 * (n - 1), m = k % p;
    return m < n ? m : p - m;
}

// K(n): the tiles along an axis of n elements
static __host__ __device__ __forceinline__ long long tiles_along(long long n, int T, int O) {
    return n <= T ? 1 : (n - O + (T - O) - 1) / (T - O);
}

template <int C>
__global__ __launch_bounds__(IB) void k_tile_in16(ssdn_tile_in16_args a) {
    __shared__ float tile[TI * CMAX][TJ + 1];
    const int b = blockIdx.z, i0 = blockIdx.y * TI, j0 = blockIdx.x * TJ;
    const int S = a.T - a.O, k = a.k0 + b;
    const int ky = k / a.Kx, ox = (k - ky * a.Kx) * S, oy = ky * S;        // (k < Kx Ky: ox < w, oy < h or the axis has one tile)
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
        if (i0 + ii < a.T && j0 + jj < a.T)                     // (r(.) < w, h and w h C <= src_count: inside the buffer)
            raw[u] = a.src[((long long)reflect(oy + j0 + jj, a.h) * a.w + reflect(ox + i0 + ii, a.w)) * C + c];
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        const int t = threadIdx.x + u * IB;
        const int jj = t / (TI * C), xb = t - jj * (TI * C);
        tile[xb][jj] = __fdiv_rn((float)min((unsigned)raw[u], white), fwhite);      // (a true division, as k_image_in16's)
    }
    __syncthreads();
    // planes: a wave stores the 64 consecutive elements of one (c, i) row
    const int lane = threadIdx.x & 63, j = j0 + lane;
#pragma unroll
    for (int u = 0; u < TI * C / (IB / 64); ++u) {
        const int r = (threadIdx.x >> 6) + u * (IB / 64);
        const int c = r / TI, ii = r - c * TI, i = i0 + ii;
        if (i < a.T && j < a.T) a.dst[(((long long)b * C + c) * a.T + i) * a.T + j] = tile[ii * C + c][lane];
    }
}

// SSDN_OP_IMAGE_OUT16's q16: clip, one product, round to nearest even; NaN -> 0.  (One product and nothing to contract it with.)
static __device__ __forceinline__ unsigned quantise16(float v, float fwhite) {
    v = v > 0.f ? v : 0.f;
    v = v < 1.f ? v : 1.f;
    return (unsigned)rintf(__fmul_rn(v, fwhite));
}

// the tiles that cover position p of an axis with K tiles: `two` -> tile kb - 1 at local d + S and tile kb at local d, blended with weight t;
// otherwise tile kb at local d alone
struct Cover {
    int kb, d;
    bool two;
    float t;
};
static __device__ __forceinline__ Cover cover(int p, int K, int S, int O) {
    Cover c;
    c.kb = min(p / S, K - 1);
    c.d = p - c.kb * S;
    c.two = c.kb >= 1 && c.d < O;
    c.t = c.two ? (float)(2 * c.d + 1) / (float)(2 * O) : 0.f;  // (a true division; O >= 32 where it is taken)
    return c;
}

// a + t (b - a), every operation rounded on its own: nothing here may be contracted into an fma.  Plain operators under this file's
// "contract(off)": __fmul_rn and __fadd_rn are operators inside a header compiled with contraction on, and fuse once they are inlined
static __device__ __forceinline__ float lerp(float a, float b, float t) {
    const float d = b - a;
    const float p = t * d;
    return a + p;
}

template <int C>
__global__ __launch_bounds__(IB) void k_tile_out16(ssdn_tile_out16_args a) {
    __shared__ unsigned tile[TI * CMAX][TJ + 1];
    const int x0 = blockIdx.y * TI, y0 = blockIdx.x * TJ;       // (x0 < w, y0 < h by the grid)
    const int T = a.T, S = a.T - a.O;
    const float fwhite = (float)a.white;
    const int lane = threadIdx.x & 63, y = y0 + lane;
    const long long plane = (long long)T * T;
    // tile side: a wave takes 64 consecutive y of one (c, x): consecutive elements of tensor axis 3 of the one or two y-tiles
    const Cover cy = cover(min(y, a.h - 1), a.Ky, S, a.O);
#pragma unroll 4
    for (int u = 0; u < TI * C / (IB / 64); ++u) {
        const int r = (threadIdx.x >> 6) + u * (IB / 64);
        const int c = r / TI, ii = r - c * TI, x = x0 + ii;
        float v = 0.f;
        if (x < a.w && y < a.h) {
            const Cover cx = cover(x, a.Kx, S, a.O);            // (wave-uniform)
            // element (c, lx, ly) of tile (kx, ky): ((((ky Kx + kx) C + c) T + lx) T + ly
            const long long row_b = ((long long)cy.kb * a.Kx + cx.kb) * C + c;              // the upper-numbered (or only) y-tile
            const long long at_b = (row_b * T + cx.d) * T + cy.d;
            const long long dxa = (long long)S * T - (long long)C * plane;                  // tile kx - 1 at local d + S, seen from tile kx
            float vb = a.store[at_b];
            if (cx.two) vb = lerp(a.store[at_b + dxa], vb, cx.t);
            v = vb;
            if (cy.two) {
                const long long at_a = at_b - (long long)a.Kx * C * plane + S;              // tile ky - 1 at local d + S
                float va = a.store[at_a];
                if (cx.two) va = lerp(a.store[at_a + dxa], va, cx.t);
                v = lerp(va, vb, cy.t);
            }
        }
        tile[ii * C + c][lane] = quantise16(v, fwhite);
    }
    __syncthreads();
    // samples: consecutive lanes take consecutive (x, c) of one image row
#pragma unroll
    for (int u = 0; u < TJ * TI * C / IB; ++u) {
        const int t = threadIdx.x + u * IB;
        const int jj = t / (TI * C), xb = t - jj * (TI * C);
        const int ii = xb / C, c = xb - ii * C;
        if (x0 + ii < a.w && y0 + jj < a.h) a.dst[((long long)(y0 + jj) * a.w + (x0 + ii)) * C + c] = (uint16_t)tile[xb][jj];
    }
}

// the checks both ops share; `op` is the prefix of the error text
static int tile_io16_check(const char* op, const void* p0, const void* p1, int C, int w, int h, int T, int O, int Kx, int Ky, int white) {
    if (!p0 || !p1) return ssdn_set_error("%s: the image and the tiles must be given", op);
    if (C != 1 && C != 3) return ssdn_set_error("%s: C must be 1 or 3", op);
    if (w < 1 || h < 1) return ssdn_set_error("%s: w and h must be at least 1", op);
    if (w > (1 << 30) || h > (1 << 30)) return ssdn_set_error("%s: w and h must be at most 2^30", op);      // (origin + T and 2 (n - 1) stay ints)
    if (T < 32 || T % 32) return ssdn_set_error("%s: T must be a positive multiple of 32", op);
    if (O < 0 || O % 32 || 2 * (long long)O > T) return ssdn_set_error("%s: O must be a multiple of 32 with 0 <= 2 O <= T", op);
    if (Kx != tiles_along(w, T, O) || Ky != tiles_along(h, T, O))
        return ssdn_set_error("%s: the grid must be Kx = %lld, Ky = %lld for this image, T and O", op, tiles_along(w, T, O), tiles_along(h, T, O));
    if ((long long)w * h * C >= (1ll << 31)) return ssdn_set_error("%s: w h C must be below 2^31", op);
    if (white < 1 || white > 65535) return ssdn_set_error("%s: white must lie in [1, 65535]", op);
    return 0;
}

int launch_tile_in16(const ssdn_tile_in16_args* a, hipStream_t s) {
    if (int rc = tile_io16_check("tile_in16", a->src, a->dst, a->C, a->w, a->h, a->T, a->O, a->Kx, a->Ky, a->white)) return rc;
    if (a->B < 1 || a->k0 < 0 || (long long)a->k0 + a->B > (long long)a->Kx * a->Ky)
        return ssdn_set_error("tile_in16: the tiles k0 .. k0 + B - 1 must lie inside the grid, B at least 1");
    if (a->src_count < (long long)a->w * a->h * a->C) return ssdn_set_error("tile_in16: src_count is below w h C");
    if (a->B > 65535 || a->T / TI > 65535) return ssdn_set_error("tile_in16: B and T / 32 must be at most 65535");
    const dim3 grid((unsigned)((a->T + TJ - 1) / TJ), (unsigned)(a->T / TI), (unsigned)a->B);
    if (a->C == 1) hipLaunchKernelGGL(k_tile_in16<1>, grid, dim3(IB), 0, s, *a);
    else hipLaunchKernelGGL(k_tile_in16<3>, grid, dim3(IB), 0, s, *a);
    return 0;
}

int launch_tile_out16(const ssdn_tile_out16_args* a, hipStream_t s) {
    if (int rc = tile_io16_check("tile_out16", a->store, a->dst, a->C, a->w, a->h, a->T, a->O, a->Kx, a->Ky, a->white)) return rc;
    if (a->dst_count < (long long)a->w * a->h * a->C) return ssdn_set_error("tile_out16: dst_count is below what the image needs");
    if ((a->w + TI - 1) / TI > 65535) return ssdn_set_error("tile_out16: the patch rows ceil(w / 32) must be at most 65535");
    const dim3 grid((unsigned)((a->h + TJ - 1) / TJ), (unsigned)((a->w + TI - 1) / TI), 1);
    if (a->C == 1) hipLaunchKernelGGL(k_tile_out16<1>, grid, dim3(IB), 0, s, *a);
    else hipLaunchKernelGGL(k_tile_out16<3>, grid, dim3(IB), 0, s, *a);
    return 0;
}
