// image_io.hip -- SSDN_OP_IMAGE_IN / SSDN_OP_IMAGE_OUT and SSDN_OP_IMAGE_IN16 / SSDN_OP_IMAGE_OUT16: whole images of differing sizes into
// and out of the engine as bytes or as uint16 samples (gfx950).  No planned list holds them.  Definition and contract: include/ssdn_hip.h;
// kernel shape and measurements: DESIGN.md section 3.16, the 16-bit sample model: section 3.20.
// An image is upright, row-major, channels interleaved (img[y][x][c], pitch w * C); the engine's tensors carry the image's x on axis 2
// and its y on axis 3 (the dataset classes' swapped H and W).  Both kernels fold that transposition through an LDS tile, so that both
// global sides are coalesced: the samples are touched along x, the fp32 planes along tensor axis 3.
// One definition of each kernel over the sample policy of sample_io.h (ByteSample: / 255, * 255 truncated; WideSample: / white, * white
// rounded) and the op's argument struct A; counts, offsets and indices are in samples.
// k_image_in:  one workgroup per (TI x TJ tile of the PADDED tensor, sample): samples -> Sample::in -> LDS (a row per (x, c)) -> fp32 planes.
// k_image_out: one workgroup per (TI x TJ tile of the EXTENT, sample): fp32 planes -> Sample::out -> LDS -> samples.
// The tile is tile[(ii * C + c)][jj], pitch TJ + 1 words: the sample side walks its first index with consecutive lanes (odd pitch: a bank
// each), the plane side its second (consecutive words).
#include "sample_io.h"

// a sample's extent, clamped to the tensor (ext is device memory: nothing on the host has seen it)
static __device__ __forceinline__ void image_extent(const int32_t* ext, int b, int H, int W, int& e1, int& e2) {
    e1 = min(max(ext[2 * b], 0), H);
    e2 = min(max(ext[2 * b + 1], 0), W);
}

// sample `idx` of the image at sample `off` lies inside the buffer of `count` samples (off is device memory too)
static __device__ __forceinline__ bool image_inside(long long off, long long idx, long long count) {
    return off >= 0 && off < count && idx < count - off;
}

template <class Sample, int C, class A>
__global__ __launch_bounds__(IB) void k_image_in(A a) {
    __shared__ float tile[TI * CMAX][TJ + 1];
    const int b = blockIdx.z, i0 = blockIdx.y * TI, j0 = blockIdx.x * TJ;
    int e1, e2;
    image_extent(a.ext, b, a.H, a.W, e1, e2);
    const long long off = a.offs[b];
    const bool any = e1 > 0 && e2 > 0;                          // (block-uniform: a sample without an extent becomes zeros)
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
        if (any && i0 + ii < a.H && j0 + jj < a.W) {
            const long long idx = ((long long)reflect(j0 + jj, e2) * e1 + reflect(i0 + ii, e1)) * C + c;
            if (image_inside(off, idx, sample_count(a))) raw[u] = a.src[off + idx];
        }
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
        if (i < a.H && j < a.W) a.dst[(((long long)b * C + c) * a.H + i) * a.W + j] = tile[ii * C + c][lane];
    }
}

template <class Sample, int C, class A>
__global__ __launch_bounds__(IB) void k_image_out(A a) {
    __shared__ unsigned tile[TI * CMAX][TJ + 1];
    const int b = blockIdx.z, i0 = blockIdx.y * TI, j0 = blockIdx.x * TJ;
    int e1, e2;
    image_extent(a.ext, b, a.H, a.W, e1, e2);
    if (i0 >= e1 || j0 >= e2) return;                           // (block-uniform: the tile lies outside the extent)
    const long long off = a.offs[b];
    const Sample sm(a);
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
        tile[ii * C + c][lane] = sm.out(v[u]);
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < TJ * TI * C / IB; ++u) {
        const int t = threadIdx.x + u * IB;
        const int jj = t / (TI * C), xb = t - jj * (TI * C);
        const int ii = xb / C, c = xb - ii * C;
        if (i0 + ii < e1 && j0 + jj < e2) {
            const long long idx = ((long long)(j0 + jj) * e1 + (i0 + ii)) * C + c;
            if (image_inside(off, idx, sample_count(a))) a.dst[off + idx] = (typename Sample::T)tile[xb][jj];
        }
    }
}

// the checks all four ops share; `op` is the prefix of the error text, `planes` the op's fp32 tensor
template <class Sample, class A>
static int image_io_check(const char* op, const A* a, const void* samples, const void* planes) {
    if (!samples || !a->offs || !a->ext || !planes) return ssdn_set_error("%s: the %s buffer, offs, ext and the tensor must be given", op, Sample::noun);
    if (a->C != 1 && a->C != 3) return ssdn_set_error("%s: C must be 1 or 3", op);
    if (a->B < 1 || a->H < 1 || a->W < 1) return ssdn_set_error("%s: B, H and W must be at least 1", op);
    if (sample_count(*a) < 0) return ssdn_set_error("%s: the %s count must not be negative", op, Sample::noun);
    if (!Sample::white_ok(*a)) return ssdn_set_error("%s: white must lie in [1, 65535]", op);
    if (a->B > 65535 || (a->H + TI - 1) / TI > 65535) return ssdn_set_error("%s: B and the tile rows must be at most 65535", op);
    return 0;
}

template <class Sample, class A>
static int image_in(const char* op, const A* a, hipStream_t s) {
    if (int rc = image_io_check<Sample>(op, a, a->src, a->dst)) return rc;
    const dim3 grid((unsigned)((a->W + TJ - 1) / TJ), (unsigned)((a->H + TI - 1) / TI), (unsigned)a->B);
    if (a->C == 1) hipLaunchKernelGGL((k_image_in<Sample, 1, A>), grid, dim3(IB), 0, s, *a);
    else hipLaunchKernelGGL((k_image_in<Sample, 3, A>), grid, dim3(IB), 0, s, *a);
    return 0;
}

template <class Sample, class A>
static int image_out(const char* op, const A* a, hipStream_t s) {
    if (int rc = image_io_check<Sample>(op, a, a->dst, a->x)) return rc;
    const dim3 grid((unsigned)((a->W + TJ - 1) / TJ), (unsigned)((a->H + TI - 1) / TI), (unsigned)a->B);
    if (a->C == 1) hipLaunchKernelGGL((k_image_out<Sample, 1, A>), grid, dim3(IB), 0, s, *a);
    else hipLaunchKernelGGL((k_image_out<Sample, 3, A>), grid, dim3(IB), 0, s, *a);
    return 0;
}

int launch_image_in(const ssdn_image_in_args* a, hipStream_t s) { return image_in<ByteSample>("image_in", a, s); }
int launch_image_out(const ssdn_image_out_args* a, hipStream_t s) { return image_out<ByteSample>("image_out", a, s); }
int launch_image_in16(const ssdn_image_in16_args* a, hipStream_t s) { return image_in<WideSample>("image_in16", a, s); }
int launch_image_out16(const ssdn_image_out16_args* a, hipStream_t s) { return image_out<WideSample>("image_out16", a, s); }
