// calibration.hip -- SSDN_OP_CALIBRATION: how well the per-pixel posterior N(mean, S) describes the errors made against the clean image, per
// sample over its un-padded extent: Mahalanobis distances, log-determinants, coverage counts, a z-score histogram and map (gfx950).  No
// planned list holds it.  Definition and contract: include/ssdn_hip.h; reasons and the reduction order: DESIGN.md section 3.15.
// Arithmetic: fp64 from the fp32 inputs with contraction off -- a pivot like s11 - l10^2 cancels, and with every product and sum rounded one
// by one the per-pixel values are those of the float64 specification (ssdn.utils.calculate_calibration), whatever the compiler schedules.
// k_calib: one pixel per thread; the pixels of a sample's extent are numbered row-major n = i * e2 + j, and workgroup k of the sample takes
//   n = k * CB .. k * CB + CB - 1 (a function of the extent alone; loads stay coalesced along W).  Its four fp64 sums go through a fixed
//   shuffle tree, its eight counts through wave ballots into LDS, all twelve into the workgroup's slot of scratch; the histogram is counted in
//   LDS and added to global memory with integer atomicAdd (order-free).
// k_calib_final: one workgroup per sample adds the slots of its extent's workgroups in a fixed order and writes stats[b].
#pragma clang fp contract(off)
#include "common.h"
#include <cmath>

static constexpr int CB = SSDN_CALIB_BLOCK, NS = SSDN_CALIB_NSTATS, NB = SSDN_CALIB_HIST_BINS;
static constexpr int NW = CB / 64;                             // waves of a block
// slots of a workgroup's partial record, in the order of stats[b]: 0, 1 and 6..11 are counts (unsigned 64-bit), 2..5 are fp64 sums
static constexpr int ND = 4, NC = 8;
static_assert(NS == ND + NC && CB % 64 == 0, "a record is 4 sums and 8 counts");

struct CalibChi2 { double q[3]; };                             // the chi^2_C quantiles at 0.5, 0.9, 0.99

// a sample's extent, clamped to the tensor (ext is device memory: nothing on the host has seen it)
static __device__ __forceinline__ void calib_extent(const ssdn_calibration_args& a, int b, int& e1, int& e2) {
    e1 = a.ext ? min(max(a.ext[2 * b], 0), a.H) : a.H;
    e2 = a.ext ? min(max(a.ext[2 * b + 1], 0), a.W) : a.W;
}

// the histogram bin of a z-score: 0: z < -4; 1 + floor(4 z + 16): -4 <= z < 4; 33: z >= 4
static __device__ __forceinline__ int calib_bin(double z) {
    if (z < -4.0) return 0;
    if (z >= 4.0) return NB - 1;
    return 1 + (int)floor(4.0 * z + 16.0);
}

template <int C>
__global__ __launch_bounds__(CB) void k_calib(ssdn_calibration_args a, CalibChi2 chi) {
    constexpr int NCOV = C * (C + 1) / 2;
    __shared__ unsigned int cnt[NC];
    __shared__ unsigned int lh[C * NB];
    __shared__ double red[ND][NW];
    const int b = blockIdx.y;
    int e1, e2;
    calib_extent(a, b, e1, e2);
    const long long n = (long long)e1 * e2;                     // (at most H * W: the launcher has bounded it)
    const long long first = (long long)blockIdx.x * CB;
    if (first >= n) return;                                     // (block-uniform: the workgroup lies outside the extent)
    if (threadIdx.x < NC) cnt[threadIdx.x] = 0u;
    for (int t = threadIdx.x; t < C * NB; t += CB) lh[t] = 0u;
    __syncthreads();
    const long long idx = first + threadIdx.x;
    const bool in = idx < n;
    const long long hw = (long long)a.H * a.W;
    bool valid = false;
    double d2 = 0.0, logdet = 0.0, rr = 0.0, tr = 0.0, z[C];
#pragma unroll
    for (int c = 0; c < C; ++c) z[c] = 0.0;
    long long off = 0;
    if (in) {
        const int i = (int)(idx / e2), j = (int)(idx - (long long)i * e2);
        off = (long long)i * a.W + j;
        double r[C], s[NCOV];
        bool fin = true;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float m = a.mean[((long long)b * C + c) * hw + off], y = a.ref[((long long)b * C + c) * hw + off];
            fin = fin && __builtin_isfinite(m) && __builtin_isfinite(y);
            r[c] = (double)y - (double)m;
        }
#pragma unroll
        for (int k = 0; k < NCOV; ++k) {
            const float v = a.cov[((long long)b * NCOV + k) * hw + off];
            fin = fin && __builtin_isfinite(v);
            s[k] = (double)v;
        }
        if constexpr (C == 3) {
            const double p0 = s[0], l00 = sqrt(p0), l10 = s[1] / l00, l20 = s[2] / l00;
            const double p1 = s[3] - l10 * l10, l11 = sqrt(p1), l21 = (s[4] - l20 * l10) / l11;
            const double p2 = (s[5] - l20 * l20) - l21 * l21, l22 = sqrt(p2);
            const double w0 = r[0] / l00, w1 = (r[1] - l10 * w0) / l11, w2 = ((r[2] - l20 * w0) - l21 * w1) / l22;
            valid = fin && p0 > 0.0 && p1 > 0.0 && p2 > 0.0 && s[3] > 0.0 && s[5] > 0.0;
            d2 = (w0 * w0 + w1 * w1) + w2 * w2;
            logdet = (log(p0) + log(p1)) + log(p2);
            rr = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
            tr = (s[0] + s[3]) + s[5];
            z[0] = r[0] / sqrt(s[0]);
            z[1] = r[1] / sqrt(s[3]);
            z[2] = r[2] / sqrt(s[5]);
        } else {
            valid = fin && s[0] > 0.0;
            d2 = (r[0] * r[0]) / s[0];
            logdet = log(s[0]);
            rr = r[0] * r[0];
            tr = s[0];
            z[0] = r[0] / sqrt(s[0]);
        }
        if (a.zmap) {
#pragma unroll
            for (int c = 0; c < C; ++c) a.zmap[((long long)b * C + c) * hw + off] = valid ? (float)z[c] : __builtin_nanf("");
        }
    }
    // the counts: one ballot per predicate and wave, lane 0 adds the wave's count to LDS (integers: order-free)
    unsigned int c1 = 0, c2 = 0, c3 = 0;                        // this pixel's channels with |z| <= 1, 2, 3
    if (valid) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const double az = fabs(z[c]);
            c1 += az <= 1.0;
            c2 += az <= 2.0;
            c3 += az <= 3.0;
            atomicAdd(&lh[c * NB + calib_bin(z[c])], 1u);
        }
    }
    const unsigned long long bv = __ballot(valid), bd = __ballot(in && !valid);
    const unsigned long long q0 = __ballot(valid && d2 <= chi.q[0]), q1 = __ballot(valid && d2 <= chi.q[1]), q2 = __ballot(valid && d2 <= chi.q[2]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {                          // (at most 3 per lane, 192 per wave)
        c1 += __shfl_down(c1, o, 64);
        c2 += __shfl_down(c2, o, 64);
        c3 += __shfl_down(c3, o, 64);
    }
    // the sums: a shuffle tree per wave, then the waves in wave order
    double v[ND] = {valid ? d2 : 0.0, valid ? logdet : 0.0, valid ? rr : 0.0, valid ? tr : 0.0};
#pragma unroll
    for (int k = 0; k < ND; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_down(v[k], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&cnt[0], (unsigned int)__popcll(bv));
        atomicAdd(&cnt[1], (unsigned int)__popcll(bd));
        atomicAdd(&cnt[2], c1);
        atomicAdd(&cnt[3], c2);
        atomicAdd(&cnt[4], c3);
        atomicAdd(&cnt[5], (unsigned int)__popcll(q0));
        atomicAdd(&cnt[6], (unsigned int)__popcll(q1));
        atomicAdd(&cnt[7], (unsigned int)__popcll(q2));
#pragma unroll
        for (int k = 0; k < ND; ++k) red[k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
    unsigned long long* slot = reinterpret_cast<unsigned long long*>(a.scratch) + ((long long)b * gridDim.x + blockIdx.x) * NS;
    if (threadIdx.x < NC) slot[threadIdx.x < 2 ? threadIdx.x : threadIdx.x + ND] = cnt[threadIdx.x];
    if (threadIdx.x >= 64 && threadIdx.x < 64 + ND) {
        const int k = threadIdx.x - 64;
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < NW; ++w) t += red[k][w];
        reinterpret_cast<double*>(slot)[2 + k] = t;
    }
    if (a.hist) {
        for (int t = threadIdx.x; t < C * NB; t += CB)
            if (lh[t]) atomicAdd(&a.hist[(long long)b * C * NB + t], (unsigned long long)lh[t]);
    }
}

// stats[b]: the records of the sample's workgroups k = 0 .. ceil(e1 e2 / CB) - 1; thread t adds k = t, t + CB, ... in that order, then the
// block's fixed tree (the counts are integers until they are stored)
__global__ __launch_bounds__(CB) void k_calib_final(ssdn_calibration_args a, int grid_blocks) {
    __shared__ double redd[ND][NW];
    __shared__ unsigned long long redu[NC][NW];
    const int b = blockIdx.x;
    int e1, e2;
    calib_extent(a, b, e1, e2);
    const long long nblk = ((long long)e1 * e2 + CB - 1) / CB;
    const unsigned long long* part = reinterpret_cast<const unsigned long long*>(a.scratch) + (long long)b * grid_blocks * NS;
    double vd[ND] = {0.0, 0.0, 0.0, 0.0};
    unsigned long long vu[NC] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (long long k = threadIdx.x; k < nblk; k += CB) {
        const unsigned long long* p = part + k * NS;
#pragma unroll
        for (int m = 0; m < ND; ++m) vd[m] += reinterpret_cast<const double*>(p)[2 + m];
#pragma unroll
        for (int m = 0; m < NC; ++m) vu[m] += p[m < 2 ? m : m + ND];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int m = 0; m < ND; ++m) vd[m] += __shfl_down(vd[m], o, 64);
#pragma unroll
        for (int m = 0; m < NC; ++m) vu[m] += __shfl_down(vu[m], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int m = 0; m < ND; ++m) redd[m][threadIdx.x >> 6] = vd[m];
#pragma unroll
        for (int m = 0; m < NC; ++m) redu[m][threadIdx.x >> 6] = vu[m];
    }
    __syncthreads();
    double* out = a.stats + (long long)b * NS;
    if (threadIdx.x < ND) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < NW; ++w) t += redd[threadIdx.x][w];
        out[2 + threadIdx.x] = t;
    } else if (threadIdx.x >= 64 && threadIdx.x < 64 + NC) {
        const int m = threadIdx.x - 64;
        unsigned long long t = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) t += redu[m][w];
        out[m < 2 ? m : m + ND] = (double)t;
    }
}

int launch_calibration(const ssdn_calibration_args* a, hipStream_t s) {
    if (!a->mean || !a->cov || !a->ref) return ssdn_set_error("calibration: mean, cov and ref must be given");
    if (!a->stats) return ssdn_set_error("calibration: the output stats must be given");
    if (a->C != 1 && a->C != 3) return ssdn_set_error("calibration: C must be 1 or 3, got %d", a->C);
    if (a->B < 1 || a->H < 1 || a->W < 1) return ssdn_set_error("calibration: B, H and W must be at least 1");
    if (!a->scratch) return ssdn_set_error("calibration: scratch must be given");
    const long long hw = (long long)a->H * a->W;
    if (a->B > 65535 || hw > 2147483647LL - CB) return ssdn_set_error("calibration: B must be at most 65535 and H * W at most 2^31 - 1 - %d", CB);
    if (a->scratch_bytes < SSDN_CALIB_SCRATCH_BYTES((long long)a->B, a->C, a->H, a->W))
        return ssdn_set_error("calibration: scratch_bytes is below SSDN_CALIB_SCRATCH_BYTES(B, C, H, W)");
    if ((uintptr_t)a->scratch & 7) return ssdn_set_error("calibration: scratch must be 8-byte aligned");
    const int blocks = (int)((hw + CB - 1) / CB);
    if (a->hist) SSDN_CHECK_HIP(hipMemsetAsync(a->hist, 0, sizeof(unsigned long long) * (size_t)a->B * a->C * NB, s));
    const dim3 grid((unsigned)blocks, (unsigned)a->B);
    if (a->C == 3) {
        const CalibChi2 chi = {SSDN_CALIB_CHI2_C3};
        hipLaunchKernelGGL(k_calib<3>, grid, dim3(CB), 0, s, *a, chi);
    } else {
        const CalibChi2 chi = {SSDN_CALIB_CHI2_C1};
        hipLaunchKernelGGL(k_calib<1>, grid, dim3(CB), 0, s, *a, chi);
    }
    hipLaunchKernelGGL(k_calib_final, dim3(a->B), dim3(CB), 0, s, *a, blocks);
    return 0;
}
