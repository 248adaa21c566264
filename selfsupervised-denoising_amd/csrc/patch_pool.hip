// patch_pool.hip -- SSDN_OP_POOL_PATCH / SSDN_OP_POOL_PATCH16: one launch cuts a whole minibatch of training patches out of a pool of uint8
// or uint16 images resident on the device (gfx950): training on images that are already noisy.  No planned list holds it.  Definition
// and contract: include/ssdn_hip.h; kernel shape and what was measured: DESIGN.md section 3.19, the 16-bit sample model: section 3.20;
// the numpy restatements are tests/patch_pool_ref.py and tests/image16_ref.py.
// The shape of k_noise (elementwise.hip): one thread per output pixel, all channels, threads along x -- an un-transposed read is a run of
// consecutive samples of one image row, the fp32 stores are consecutive.  A pure gather: no atomics, no LDS, nothing kept between launches.
// Every draw is integer arithmetic on one Philox block per sample; the only float operation on the value path is one true division.
// One kernel over the sample policy of sample_io.h and the op's argument struct A: the draws, crop, transform and Noise2Void selection do
// not see the sample, so for equal (seed, offset, sizes, index) both ops give equal origin_out and coords.  Offsets are in samples.
#include "sample_io.h"     // ByteSample, WideSample, reflect, n2v_pick
#include "philox.h"        // Ph4, philox4x32_10, u01

// the streams of elementwise.hip's SSDN_OP_NOISE, and this op's own
enum { NS_COORD = 3, NS_CROP = 5 };

// patch coordinate (px, py) of a sample with origin (x0, y0) and transform d -> (column, row) of its image
static __device__ __forceinline__ void pool_source(int px, int py, int P, int d, int x0, int y0, int rows, int cols, int& col, int& row) {
    int u = px, v = py;
    if (d & 1) { const int t = u; u = v; v = t; }
    if (d & 2) u = P - 1 - u;
    if (d & 4) v = P - 1 - v;
    col = reflect(x0 + u, cols);
    row = reflect(y0 + v, rows);
}

template <class Sample, class A>
__global__ void k_pool_patch(A a) {
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
            rx = n2v_pick(c0, a.n2v_radius, P, u01(r.v[2]));
            ry = n2v_pick(c1, a.n2v_radius, P, u01(r.v[3]));
            a.coords[((long long)b * n1 * n1 + cell) * 2 + 0] = c0;
            a.coords[((long long)b * n1 * n1 + cell) * 2 + 1] = c1;
        }
    }
    int col, row, ncol, nrow;
    pool_source(x, y, P, d, x0, y0, rows, cols, col, row);        // (col < cols, row < rows: inside the image)
    pool_source(rx, ry, P, d, x0, y0, rows, cols, ncol, nrow);    // (0 <= rx, ry < P by n2v_pick)
    const typename Sample::T* src = a.pool + a.offsets[img];
    const Sample sm(a);
    const float par = a.params ? a.params[img] : 0.f;
    for (int c = 0; c < a.C; ++c) {
        const long long plane = (long long)c * rows;
        const unsigned e = (unsigned)((b * a.C + c) * PP + y * P + x);
        const float own = sm.in(src[(plane + row) * cols + col]);
        const float val = (rx == x && ry == y) ? own : sm.in(src[(plane + nrow) * cols + ncol]);
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

// `op` is the prefix of the error text
template <class Sample, class A>
static int pool_patch(const char* op, const A* a, hipStream_t s) {
    if (!a->pool || !a->offsets || !a->sizes || !a->index || !a->noisy32)
        return ssdn_set_error("%s: pool, offsets, sizes, index and noisy32 are required", op);
    if (a->N < 1 || a->B < 1 || a->C < 1 || a->P < 1) return ssdn_set_error("%s: empty shape", op);
    const long long n = (long long)a->B * a->C * a->P * a->P;
    if (n >= (1ll << 31)) return ssdn_set_error("%s: too many elements for 32-bit indexing", op);
    if (!Sample::white_ok(*a)) return ssdn_set_error("%s: white must lie in [1, 65535]", op);
    if (a->param_out && !a->params) return ssdn_set_error("%s: param_out needs the params table", op);
    if (a->n2v_box > 0) {
        if (!a->coords) return ssdn_set_error("%s: Noise2Void manipulation needs a coords output", op);
        if (a->P % a->n2v_box) return ssdn_set_error("%s: P must be a multiple of n2v_box", op);
        if (a->n2v_radius < 1 || a->P < 2) return ssdn_set_error("%s: n2v_radius must be >= 1 and the patch larger than 1 pixel", op);
        if (a->n2v_radius > a->P) return ssdn_set_error("%s: n2v_radius must be at most P", op);       // (a wrapped neighbour stays inside the patch)
    }
    constexpr int BLOCK = 256;
    const long long px = (long long)a->B * a->P * a->P;
    hipLaunchKernelGGL((k_pool_patch<Sample, A>), dim3((unsigned)((px + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, *a);
    return 0;
}

int launch_pool_patch(const ssdn_pool_patch_args* a, hipStream_t s) { return pool_patch<ByteSample>("pool_patch", a, s); }
int launch_pool_patch16(const ssdn_pool_patch16_args* a, hipStream_t s) { return pool_patch<WideSample>("pool_patch16", a, s); }
