// noise_est.hip -- SSDN_OP_NOISE_EST: a blind per-image noise-level estimate from the bytes SSDN_OP_IMAGE_IN reads (gfx950).
// No planned list holds it.  Definition and contract: include/ssdn_hip.h (ssdn.utils.estimate_noise is the same text in float64 torch);
// kernel shape and measurements: DESIGN.md section 3.17.
// k_noise_est:       one workgroup per (TX x TY tile of window centres in image space, sample): the tile's bytes and a one-pixel halo ->
//                    LDS, per 3x3 window Immerkaer's response r, the byte sum S and validity -> an LDS table hist[8][1024] and eight class
//                    sums -> the non-zero entries into the sample's global table with integer atomics.  Integer adds commute: the table
//                    is the same bits whatever the order of the workgroups.
// k_noise_est_final: one workgroup per sample: prefix sums of the pooled and the eight per-class histograms, their grouped medians, the
//                    estimates in fp64, each product, quotient and sum rounded on its own.
#pragma clang fp contract(off)
#include "common.h"

static constexpr int TX = 64, TY = 32;                         // tile of window centres: image x, image y
static constexpr int NB = 1024;                                // threads of a counting block: sixteen waves share the tile's latencies
static constexpr int NF = 256;                                 // threads of the final block
static constexpr int NCLS = 8, NBIN = 1024;                    // intensity classes, bins of |r|
static constexpr int NEST = 20;                                // doubles of one sample's estimate
static constexpr int NMIN = 256;                               // fewer valid windows give no estimate
static_assert((TX * TY) % NB == 0 && (NCLS * NBIN) % NB == 0, "every thread takes the same number of windows and of bins");
static_assert(NBIN == 4 * NF, "k_noise_est_final gives every thread four consecutive bins");

// byte `idx` of the image at `off` lies inside the buffer of `bytes` bytes (image_io.hip's guard: off is device memory)
static __device__ __forceinline__ bool est_inside(long long off, long long idx, long long bytes) {
    return off >= 0 && off < bytes && idx < bytes - off;
}

template <int C>
__global__ __launch_bounds__(NB) void k_noise_est(ssdn_noise_est_args a) {
    constexpr int ROWB = (TX + 2) * C;                          // bytes of one staged row: the tile's columns and one pixel either side
    constexpr int NST = ROWB * (TY + 2);
    constexpr int NLD = (NST + NB - 1) / NB;
    __shared__ unsigned lh[NCLS * NBIN];
    __shared__ unsigned lsum[NCLS];
    __shared__ unsigned char st[NLD * NB];
    const int b = blockIdx.z, x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
    const int w = min(max(a.ext[2 * b], 0), a.H), h = min(max(a.ext[2 * b + 1], 0), a.W);       // (ext = (w_b, h_b), clamped as image_in does)
    if (w < 3 || h < 3 || x0 > w - 2 || y0 > h - 2) return;     // (block-uniform: no window centre of the extent lies in the tile)
    const long long off = a.offs[b];
    // bytes: consecutive lanes take consecutive bytes of one image row; every load of the thread is issued before the first is used.
    // A byte outside the image or the buffer is staged as 0, which no valid window holds
    unsigned char raw[NLD];
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
        const int t = threadIdx.x + u * NB;
        const int sy = t / ROWB, sb = t - sy * ROWB;
        const int y = y0 - 1 + sy, xb = (x0 - 1) * C + sb;
        raw[u] = 0;
        if (t < NST && y >= 0 && y < h && xb >= 0 && xb < w * C) {
            const long long idx = ((long long)y * w) * C + xb;
            if (est_inside(off, idx, a.src_bytes)) raw[u] = a.src[off + idx];
        }
    }
#pragma unroll
    for (int u = 0; u < NCLS * NBIN / NB; ++u) lh[threadIdx.x + u * NB] = 0;
    if (threadIdx.x < NCLS) lsum[threadIdx.x] = 0;
#pragma unroll
    for (int u = 0; u < NLD; ++u) st[threadIdx.x + u * NB] = raw[u];
    __syncthreads();
    // windows: consecutive lanes take consecutive (x, c) of one row of centres
    unsigned acc[NCLS];
#pragma unroll
    for (int g = 0; g < NCLS; ++g) acc[g] = 0;
#pragma unroll
    for (int u = 0; u < TX * TY * C / NB; ++u) {
        const int t = threadIdx.x + u * NB;
        const int yy = t / (TX * C), xc = t - yy * (TX * C);
        const int x = x0 + xc / C, y = y0 + yy;
        if (x < 1 || x > w - 2 || y < 1 || y > h - 2) continue;
        const unsigned char* p = st + (yy + 1) * ROWB + xc + C;    // the window's centre
        int r = 0, S = 0;
        bool valid = true;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int v = p[dy * ROWB + dx * C];
                r += (dy ? -2 : 4) * (dx ? -2 : 4) / 4 * v;         // K = [[1,-2,1],[-2,4,-2],[1,-2,1]]
                S += v;
                valid = valid && (unsigned)(v - 1) <= 253u;         // 0 and 255 may be clipped values
            }
        if (!valid) continue;
        const int g = (S / 9) >> 5, k = min(abs(r), NBIN - 1);
        atomicAdd(&lh[g * NBIN + k], 1u);
#pragma unroll
        for (int q = 0; q < NCLS; ++q) acc[q] += q == g ? (unsigned)S : 0u;
    }
    // class sums: a wave's 64 lanes added in registers, one LDS atomic per wave and class (at most 2048 C windows of at most 2286 each)
#pragma unroll
    for (int g = 0; g < NCLS; ++g) {
        unsigned v = acc[g];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&lsum[g], v);
    }
    __syncthreads();
    uint32_t* hist = a.hist + (long long)b * (NCLS * NBIN);
#pragma unroll 4
    for (int u = 0; u < NCLS * NBIN / NB; ++u) {
        const int i = threadIdx.x + u * NB;
        const unsigned v = lh[i];
        if (v) atomicAdd(&hist[i], v);
    }
    if (threadIdx.x < NCLS && lsum[threadIdx.x])
        atomicAdd((unsigned long long*)a.ssum + (long long)b * NCLS + threadIdx.x, (unsigned long long)lsum[threadIdx.x]);
}

// the grouped median of a histogram of total N from its median bin k, the count below it and the bin's own count
static __device__ __forceinline__ double grouped_median(unsigned long long N, int k, unsigned long long below, unsigned long long qk) {
    if (N == 0 || k >= NBIN - 1) return __builtin_nan("");     // (the clamp bin has no upper edge)
    const double half = (double)N / 2.0;
    const double lo = k > 0 ? (double)k - 0.5 : 0.0, hi = (double)k + 0.5;
    return lo + (hi - lo) * (half - (double)below) / (double)qk;
}

__global__ __launch_bounds__(NF) void k_noise_est_final(ssdn_noise_est_args a) {
    constexpr int NH = NCLS + 1;                                // the eight per-class histograms and, as number NCLS, the pooled one
    __shared__ unsigned long long scan[2][NH][NF];
    __shared__ unsigned long long found[NH][4];                 // per histogram: N, k*, the count below it, the bin's count
    const int b = blockIdx.x, tid = threadIdx.x;
    const uint32_t* hist = a.hist + (long long)b * (NCLS * NBIN);
    // four consecutive bins of every class per thread, all loads issued before the first is used
    uint4 q[NCLS];
#pragma unroll
    for (int g = 0; g < NCLS; ++g) q[g] = *(const uint4*)(hist + g * NBIN + 4 * tid);
    if (tid < NH) found[tid][0] = 0, found[tid][1] = NBIN - 1, found[tid][2] = 0, found[tid][3] = 0;
    // inclusive scans of the threads' sums, all nine at once (Hillis-Steele through two LDS rows per histogram)
    unsigned long long incl[NH], own[NH];
    incl[NCLS] = 0;
#pragma unroll
    for (int g = 0; g < NCLS; ++g) {
        incl[g] = (unsigned long long)q[g].x + q[g].y + q[g].z + q[g].w;
        incl[NCLS] += incl[g];
    }
#pragma unroll
    for (int hq = 0; hq < NH; ++hq) own[hq] = incl[hq], scan[0][hq][tid] = incl[hq];
    __syncthreads();
    int cur = 0;
#pragma unroll
    for (int d = 1; d < NF; d <<= 1) {
#pragma unroll
        for (int hq = 0; hq < NH; ++hq) {
            if (tid >= d) incl[hq] += scan[cur][hq][tid - d];
            scan[cur ^ 1][hq][tid] = incl[hq];
        }
        cur ^= 1;
        __syncthreads();
    }
    // k* is the smallest k with 2 cum(k) >= N: it lies in exactly one thread's four bins (N > 0)
#pragma unroll
    for (int hq = 0; hq < NH; ++hq) {
        const unsigned long long N = scan[cur][hq][NF - 1];
        if (tid == 0) found[hq][0] = N;
        unsigned long long below = incl[hq] - own[hq];
        if (N > 0 && 2 * below < N && 2 * incl[hq] >= N) {
            unsigned long long v[4] = {0, 0, 0, 0};
            if (hq < NCLS) {
                const uint4 qq = q[hq < NCLS ? hq : 0];
                v[0] = qq.x, v[1] = qq.y, v[2] = qq.z, v[3] = qq.w;
            } else {
#pragma unroll
                for (int g = 0; g < NCLS; ++g) v[0] += q[g].x, v[1] += q[g].y, v[2] += q[g].z, v[3] += q[g].w;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (2 * (below + v[j]) >= N) {
                    found[hq][1] = 4 * tid + j, found[hq][2] = below, found[hq][3] = v[j];
                    break;
                }
                below += v[j];
            }
        }
    }
    __syncthreads();
    if (tid != 0) return;
    const double nan = __builtin_nan("");
    const double c = 6.0 * 0.6744897501960817;                 // |r| has sd 6 sigma; the median of |N(0,1)| is 0.6744...
    double* est = a.est + (long long)b * NEST;
    const unsigned long long n = found[NCLS][0];
    double sigma = nan;
    if (n >= NMIN) {
        sigma = grouped_median(n, (int)found[NCLS][1], found[NCLS][2], found[NCLS][3]) / c;
        sigma = sigma < 0.5 ? 0.5 : sigma;                       // (NaN stays NaN)
    }
    double num = 0.0, den = 0.0;
    int used = 0;
    for (int g = 0; g < NCLS; ++g) {
        const unsigned long long ng = found[g][0];
        double sg = nan, mg = nan;
        if (ng >= NMIN) {
            sg = grouped_median(ng, (int)found[g][1], found[g][2], found[g][3]) / c;
            mg = (double)a.ssum[(long long)b * NCLS + g] / (9.0 * (double)ng);
            const double nm = (double)ng * mg;
            num = num + nm * mg;
            den = den + nm * (sg * sg);
            ++used;
        }
        est[4 + g] = sg;
        est[4 + NCLS + g] = mg;
    }
    double lambda = nan;
    if (used) {
        lambda = den == 0.0 ? 260100.0 : 255.0 * num / den;
        lambda = lambda > 260100.0 ? 260100.0 : lambda;          // (NaN stays NaN)
    }
    est[0] = sigma, est[1] = lambda, est[2] = (double)n, est[3] = (double)used;
    if (a.param) a.param[b] = a.kind == 0 ? (float)(sigma / 255.0) : (float)lambda;
}

int launch_noise_est(const ssdn_noise_est_args* a, hipStream_t s) {
    if (!a->src || !a->offs || !a->ext || !a->hist || !a->ssum || !a->est)
        return ssdn_set_error("noise_est: the byte buffer, offs, ext, hist, ssum and est must be given");
    if (a->C != 1 && a->C != 3) return ssdn_set_error("noise_est: C must be 1 or 3");
    if (a->B < 1 || a->H < 1 || a->W < 1) return ssdn_set_error("noise_est: B, H and W must be at least 1");
    if (a->src_bytes < 0) return ssdn_set_error("noise_est: the byte count must not be negative");
    if (a->kind != 0 && a->kind != 1) return ssdn_set_error("noise_est: kind must be 0 (gauss) or 1 (poisson)");
    if ((uintptr_t)a->hist & 15) return ssdn_set_error("noise_est: hist must be 16-byte aligned");
    if (a->B > 65535 || (a->W + TY - 1) / TY > 65535) return ssdn_set_error("noise_est: B and the tile rows must be at most 65535");
    // the tables are accumulated into: zeroed on the op's own stream, so that a repeated launch gives the same bytes
    SSDN_CHECK_HIP(hipMemsetAsync(a->hist, 0, sizeof(uint32_t) * NCLS * NBIN * (size_t)a->B, s));
    SSDN_CHECK_HIP(hipMemsetAsync(a->ssum, 0, sizeof(uint64_t) * NCLS * (size_t)a->B, s));
    const dim3 grid((unsigned)((a->H + TX - 1) / TX), (unsigned)((a->W + TY - 1) / TY), (unsigned)a->B);     // (H bounds the image's x)
    if (a->C == 1) hipLaunchKernelGGL(k_noise_est<1>, grid, dim3(NB), 0, s, *a);
    else hipLaunchKernelGGL(k_noise_est<3>, grid, dim3(NB), 0, s, *a);
    hipLaunchKernelGGL(k_noise_est_final, dim3((unsigned)a->B), dim3(NF), 0, s, *a);
    return 0;
}
