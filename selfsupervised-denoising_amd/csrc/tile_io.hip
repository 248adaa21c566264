// tile_io.hip -- SSDN_OP_TILE_IN / SSDN_OP_TILE_OUT and SSDN_OP_TILE_IN16 / SSDN_OP_TILE_OUT16: one image of any size, of bytes or of
// uint16 samples, into fixed-size overlapping tiles and the tiles' results back into one image, blended across the overlaps (gfx950).  No
// planned list holds them.  Definition and contract: include/ssdn_hip.h; kernel shape and measurements: DESIGN.md section 3.18, the
// 16-bit sample model: section 3.20.
// The image is upright img[y][x][c] (pitch w * C), as SSDN_OP_IMAGE_IN reads it; a tile is a [C,T,T] fp32 block in the package's
// swapped axes (axis 2 along x, axis 3 along y).  Both kernels fold that transposition through an LDS tile as image_io.hip does: the image
// side is touched along x, the tile side along tensor axis 3.  One definition of each kernel over the sample policy of sample_io.h and
// the op's argument struct A; counts and indices are in samples.
// k_tile_in:  one workgroup per (TI x TJ patch of a tile, tile of the batch): samples -> Sample::in -> LDS -> fp32 planes.
// k_tile_out: one workgroup per (TI x TJ patch of the IMAGE): up to four store values per element -> blend -> LDS -> Sample::out samples
//             (mode 0) or upright fp32 planes (mode 1, the byte struct's only).  Gather form: every output element has one writer;
//             nothing is accumulated.
// The grid of tiles is arithmetic on (T, O, w, h): there are no device tables, so every index is derived from arguments the host has checked.
// The blend's difference, product and sum are rounded one by one, so contraction is off for the whole file (see lerp).
#pragma clang fp contract(off)
#include "sample_io.h"

// K(n): the tiles along an axis of n elements
static __host__ __device__ __forceinline__ long long tiles_along(long long n, int T, int O) {
    return n <= T ? 1 : (n - O + (T - O) - 1) / (T - O);
}

template <class Sample, int C, class A>
__global__ __launch_bounds__(IB) void k_tile_in(A a) {
    __shared__ float tile[TI * CMAX][TJ + 1];
    const int b = blockIdx.z, i0 = blockIdx.y * TI, j0 = blockIdx.x * TJ;
    const int S = a.T - a.O, k = a.k0 + b;
    const int ky = k / a.Kx, ox = (k - ky * a.Kx) * S, oy = ky * S;        // (k < Kx Ky: ox < w, oy < h or the axis has one tile)
    const Sample sm(a);
    // samples: consecutive lanes take consecutive (x, c) of one image row; every load of the thread is issued before the first is used
    constexpr int NB = TJ * TI * C / IB;
    typename Sample::T raw[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        const int t = threadIdx.x + u * IB;
        const int jj = t / (TI * C), xb = t - jj * (TI * C);
        const int ii = xb / C, c = xb - ii * C;
        raw[u] = 0;
        if (i0 + ii < a.T && j0 + jj < a.T)                     // (r(.) < w, h and w h C <= the count: inside the buffer)
            raw[u] = a.src[((long long)reflect(oy + j0 + jj, a.h) * a.w + reflect(ox + i0 + ii, a.w)) * C + c];
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) {
        const int t = threadIdx.x + u * IB;
        const int jj = t / (TI * C), xb = t - jj * (TI * C);
        tile[xb][jj] = sm.in(raw[u]);
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

template <class Sample, int C, int MODE, class A>
__global__ __launch_bounds__(IB) void k_tile_out(A a) {
    __shared__ unsigned tile[TI * CMAX][TJ + 1];
    const int x0 = blockIdx.y * TI, y0 = blockIdx.x * TJ;       // (x0 < w, y0 < h by the grid)
    const int T = a.T, S = a.T - a.O;
    const Sample sm(a);
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
        tile[ii * C + c][lane] = MODE == 0 ? sm.out(v) : __float_as_uint(v);
    }
    __syncthreads();
    if (MODE == 0) {
        // samples: consecutive lanes take consecutive (x, c) of one image row
        typedef typename Sample::T ST;
        ST* dst = (ST*)a.dst;
#pragma unroll
        for (int u = 0; u < TJ * TI * C / IB; ++u) {
            const int t = threadIdx.x + u * IB;
            const int jj = t / (TI * C), xb = t - jj * (TI * C);
            const int ii = xb / C, c = xb - ii * C;
            if (x0 + ii < a.w && y0 + jj < a.h) dst[((long long)(y0 + jj) * a.w + (x0 + ii)) * C + c] = (ST)tile[xb][jj];
        }
    } else {
        // upright planes: consecutive lanes take consecutive x of one (c, y) row
        float* dst = (float*)a.dst;
#pragma unroll
        for (int u = 0; u < TJ * TI * C / IB; ++u) {
            const int t = threadIdx.x + u * IB;
            const int ii = t % TI, rest = t / TI;
            const int jj = rest % TJ, c = rest / TJ;
            if (x0 + ii < a.w && y0 + jj < a.h) dst[((long long)c * a.h + (y0 + jj)) * a.w + (x0 + ii)] = __uint_as_float(tile[ii * C + c][jj]);
        }
    }
}

// the checks all four ops share; `op` is the prefix of the error text, p0 and p1 the op's image and tiles
template <class Sample, class A>
static int tile_io_check(const char* op, const A* a, const void* p0, const void* p1) {
    const int C = a->C, w = a->w, h = a->h, T = a->T, O = a->O, Kx = a->Kx, Ky = a->Ky;
    if (!p0 || !p1) return ssdn_set_error("%s: the image and the tiles must be given", op);
    if (C != 1 && C != 3) return ssdn_set_error("%s: C must be 1 or 3", op);
    if (w < 1 || h < 1) return ssdn_set_error("%s: w and h must be at least 1", op);
    if (w > (1 << 30) || h > (1 << 30)) return ssdn_set_error("%s: w and h must be at most 2^30", op);      // (origin + T and 2 (n - 1) stay ints)
    if (T < 32 || T % 32) return ssdn_set_error("%s: T must be a positive multiple of 32", op);
    if (O < 0 || O % 32 || 2 * (long long)O > T) return ssdn_set_error("%s: O must be a multiple of 32 with 0 <= 2 O <= T", op);
    if (Kx != tiles_along(w, T, O) || Ky != tiles_along(h, T, O))
        return ssdn_set_error("%s: the grid must be Kx = %lld, Ky = %lld for this image, T and O", op, tiles_along(w, T, O), tiles_along(h, T, O));
    if ((long long)w * h * C >= (1ll << 31)) return ssdn_set_error("%s: w h C must be below 2^31", op);
    if (!Sample::white_ok(*a)) return ssdn_set_error("%s: white must lie in [1, 65535]", op);
    return 0;
}

template <class Sample, class A>
static int tile_in(const char* op, const A* a, hipStream_t s) {
    if (int rc = tile_io_check<Sample>(op, a, a->src, a->dst)) return rc;
    if (a->B < 1 || a->k0 < 0 || (long long)a->k0 + a->B > (long long)a->Kx * a->Ky)
        return ssdn_set_error("%s: the tiles k0 .. k0 + B - 1 must lie inside the grid, B at least 1", op);
    if (sample_count(*a) < (long long)a->w * a->h * a->C) return ssdn_set_error("%s: src_%s is below w h C", op, Sample::field);
    if (a->B > 65535 || a->T / TI > 65535) return ssdn_set_error("%s: B and T / 32 must be at most 65535", op);
    const dim3 grid((unsigned)((a->T + TJ - 1) / TJ), (unsigned)(a->T / TI), (unsigned)a->B);
    if (a->C == 1) hipLaunchKernelGGL((k_tile_in<Sample, 1, A>), grid, dim3(IB), 0, s, *a);
    else hipLaunchKernelGGL((k_tile_in<Sample, 3, A>), grid, dim3(IB), 0, s, *a);
    return 0;
}

int launch_tile_in(const ssdn_tile_in_args* a, hipStream_t s) { return tile_in<ByteSample>("tile_in", a, s); }
int launch_tile_in16(const ssdn_tile_in16_args* a, hipStream_t s) { return tile_in<WideSample>("tile_in16", a, s); }

// the patch grid over the image, after tile_io_check; MODE 1 is the byte struct's alone
template <class Sample, int MODE, class A>
static int tile_out(const char* op, const A* a, hipStream_t s) {
    if ((a->w + TI - 1) / TI > 65535) return ssdn_set_error("%s: the patch rows ceil(w / 32) must be at most 65535", op);
    const dim3 grid((unsigned)((a->h + TJ - 1) / TJ), (unsigned)((a->w + TI - 1) / TI), 1);
    if (a->C == 1) hipLaunchKernelGGL((k_tile_out<Sample, 1, MODE, A>), grid, dim3(IB), 0, s, *a);
    else hipLaunchKernelGGL((k_tile_out<Sample, 3, MODE, A>), grid, dim3(IB), 0, s, *a);
    return 0;
}

int launch_tile_out(const ssdn_tile_out_args* a, hipStream_t s) {
    if (int rc = tile_io_check<ByteSample>("tile_out", a, a->store, a->dst)) return rc;
    if (a->mode != 0 && a->mode != 1) return ssdn_set_error("tile_out: mode must be 0 (bytes) or 1 (fp32 planes)");
    if (a->dst_bytes < (long long)a->w * a->h * a->C * (a->mode ? 4 : 1)) return ssdn_set_error("tile_out: dst_bytes is below what the image needs");
    return a->mode == 0 ? tile_out<ByteSample, 0>("tile_out", a, s) : tile_out<ByteSample, 1>("tile_out", a, s);
}

int launch_tile_out16(const ssdn_tile_out16_args* a, hipStream_t s) {
    if (int rc = tile_io_check<WideSample>("tile_out16", a, a->store, a->dst)) return rc;
    if (a->dst_count < (long long)a->w * a->h * a->C) return ssdn_set_error("tile_out16: dst_count is below what the image needs");
    return tile_out<WideSample, 0>("tile_out16", a, s);
}
