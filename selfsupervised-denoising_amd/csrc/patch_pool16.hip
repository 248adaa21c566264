// patch_pool16.hip -- SSDN_OP_POOL_PATCH16: one launch cuts a whole minibatch of training patches out of a pool of uint16 images resident
// on the device (gfx950): training on 16-bit images that are already noisy.  No planned list holds it.  Definition and contract:
// include/ssdn_hip.h; the sample model and what was measured: DESIGN.md section 3.20; the numpy restatement is tests/image16_ref.py.
// The kernel is patch_pool.hip's with a sample of two bytes and value = min(s, white) / white: the same draws, crop, transform and
// Noise2Void selection, so for equal (seed, offset, sizes, index) both ops give equal origin_out and coords.  Offsets are in SAMPLES; the
// byte kernel and its file stay as they are.
#include "common.h"
#include "philox.h"        // Ph4, philox4x32_10, u01

// the streams of elementwise.hip's SSDN_OP_NOISE, and this op's own
enum { NS_COORD = 3, NS_CROP = 5 };

// numpy's "reflect" iterated to any length: index t >= 0 of an axis of n >= 1 elements
static __device__ __forceinline__ int pool_reflect(int t, int n) {
    if (t < n) return t;
    if (n == 1) return 0;
    const int p = 2 * n - 2, m = t % p;
    return m < n ? m : p - m;
}

// n2v_pick of elementwise.hip, restated as in patch_pool.hip (each file's helpers are static to it and stay where they are): a uniform integer over [lo, hi)
// without c; negative results wrap
static __device__ __forceinline__ int pool_n2v_pick(int c, int r, int size, float u) {
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

// patch coordinate (px, py) of a sample with origin (x0, y0) and transform d -> (column, row) of its image
static __device__ __forceinline__ void pool_source(int px, int py, int P, int d, int x0, int y0, int rows, int cols, int& col, int& row) {
    int u = px, v = py;
    if (d & 1) { const int t = u; u = v; v = t; }
    if (d & 2) u = P - 1 - u;
    if (d & 4) v = P - 1 - v;
    col = pool_reflect(x0 + u, cols);
    row = pool_reflect(y0 + v, rows);
}

__global__ void k_pool_patch16(ssdn_pool_patch16_args a) {
    const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int P = a.P, PP = P * P;
    if (idx >= (unsigned)(a.B * PP)) return;
    const int x = idx % P, y = (idx / P) % P, b = idx / PP;
    const int img = a.index[b];                                   // (0 <= img < N: the host checked before upload)
    const int rows = a.sizes[2 * img], cols = a.sizes[2 * img + 1];
    const unsigned o_lo = (unsigned)a.offset, o_hi = (unsigned)(a.offset >> 32), k_lo = (unsigned)a.seed, k_hi = (unsigned)(a.seed >> 32);
    const Ph4 cr = philox4x32_10((unsigned)b, NS_CROP, o_lo, o_hi, k_lo, k_hi);
    const int x0 = (int)__umulhi(cr.v[0], (unsigned)((cols > P ? cols - P : 0) + 1));
    const int y0 = (int)__umulhi(cr.v[1], (unsigned)((rows > P ? rows - P : 0) + 1));
    const int d = a.augment ? (int)(cr.v[2] >> 29) : 0;
    // Noise2Void: is (x, y) the selected pixel of its box, and if so which neighbour does it copy?  (k_noise's selection, H = W = P)
    int rx = x, ry = y;
    if (a.n2v_box > 0) {
        const int box = a.n2v_box, n1 = P / box, i = x / box, j = y / box, cell = i * n1 + j;
        const unsigned ce = (unsigned)(b * n1 * n1 + cell);
        const Ph4 r = philox4x32_10(ce, NS_COORD, o_lo, o_hi, k_lo, k_hi);
        int c0 = i * box + (int)(u01(r.v[0]) * (float)box), c1 = j * box + (int)(u01(r.v[1]) * (float)box);
        c0 = c0 > i * box + box - 1 ? i * box + box - 1 : c0;
        c1 = c1 > j * box + box - 1 ? j * box + box - 1 : c1;
        if (c0 == x && c1 == y) {
            rx = pool_n2v_pick(c0, a.n2v_radius, P, u01(r.v[2]));
            ry = pool_n2v_pick(c1, a.n2v_radius, P, u01(r.v[3]));
            a.coords[((long long)b * n1 * n1 + cell) * 2 + 0] = c0;
            a.coords[((long long)b * n1 * n1 + cell) * 2 + 1] = c1;
        }
    }
    int col, row, ncol, nrow;
    pool_source(x, y, P, d, x0, y0, rows, cols, col, row);        // (col < cols, row < rows: inside the image)
    pool_source(rx, ry, P, d, x0, y0, rows, cols, ncol, nrow);    // (0 <= rx, ry < P by pool_n2v_pick)
    const uint16_t* src = a.pool + a.offsets[img];
    const unsigned white = (unsigned)a.white;
    const float fwhite = (float)a.white;
    const float par = a.params ? a.params[img] : 0.f;
    for (int c = 0; c < a.C; ++c) {
        const long long plane = (long long)c * rows;
        const unsigned e = (unsigned)((b * a.C + c) * PP + y * P + x);
        const float own = __fdiv_rn((float)min((unsigned)src[(plane + row) * cols + col], white), fwhite);      // (a true division; above white is 1.0)
        const float val = (rx == x && ry == y) ? own : __fdiv_rn((float)min((unsigned)src[(plane + nrow) * cols + ncol], white), fwhite);
        a.noisy32[e] = val;
        if (a.ref32) a.ref32[e] = own;
        if (a.param_out && x == 0 && y == 0) a.param_out[b * a.C + c] = par;
    }
    if (a.origin_out && x == 0 && y == 0) {
        a.origin_out[3 * b + 0] = x0;
        a.origin_out[3 * b + 1] = y0;
        a.origin_out[3 * b + 2] = d;
    }
}

int launch_pool_patch16(const ssdn_pool_patch16_args* a, hipStream_t s) {
    if (!a->pool || !a->offsets || !a->sizes || !a->index || !a->noisy32)
        return ssdn_set_error("pool_patch16: pool, offsets, sizes, index and noisy32 are required");
    if (a->N < 1 || a->B < 1 || a->C < 1 || a->P < 1) return ssdn_set_error("pool_patch16: empty shape");
    const long long n = (long long)a->B * a->C * a->P * a->P;
    if (n >= (1ll << 31)) return ssdn_set_error("pool_patch16: too many elements for 32-bit indexing");
    if (a->white < 1 || a->white > 65535) return ssdn_set_error("pool_patch16: white must lie in [1, 65535]");
    if (a->param_out && !a->params) return ssdn_set_error("pool_patch16: param_out needs the params table");
    if (a->n2v_box > 0) {
        if (!a->coords) return ssdn_set_error("pool_patch16: Noise2Void manipulation needs a coords output");
        if (a->P % a->n2v_box) return ssdn_set_error("pool_patch16: P must be a multiple of n2v_box");
        if (a->n2v_radius < 1 || a->P < 2) return ssdn_set_error("pool_patch16: n2v_radius must be >= 1 and the patch larger than 1 pixel");
        if (a->n2v_radius > a->P) return ssdn_set_error("pool_patch16: n2v_radius must be at most P");       // (a wrapped neighbour stays inside the patch)
    }
    constexpr int BLOCK = 256;
    const long long px = (long long)a->B * a->P * a->P;
    hipLaunchKernelGGL(k_pool_patch16, dim3((unsigned)((px + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, *a);
    return 0;
}
