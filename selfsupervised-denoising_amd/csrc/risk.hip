// risk.hip -- SSDN_OP_RISK: judge a model without the clean image (gfx950).  No planned list holds it.
// The blind-spot prior (mu_x, Sigma_x) at a pixel is a function of the other pixels only, and the gauss / poisson heads deliver
// out = mu_x + W (y - mu_x), W = Sigma_x (Sigma_x + Sigma_n)^-1, affine in the pixel's own noisy value y with W independent of it.  For
// zero-mean noise, independent across pixels and channels, of variance v_c:
//     E|mu_x - x|^2 = E[ |mu_x - y|^2 - sum_c v_c ]          E|out - x|^2 = E[ |out - y|^2 + sum_c (2 W_cc - 1) v_c ]
// so both errors have unbiased estimates from the noisy image alone (poisson: v_c = x_c / lambda has the stand-in y_c / lambda).
// Definition (ssdn.utils.calculate_risk is the float64 specification; the contract is in include/ssdn_hip.h), per pixel in fp64 from the
// fp32 inputs, T = Sigma_x + diag(n_c), d = y - mu, in this fixed order (C = 3):
//     p0 = t00, l00 = sqrt(p0), l10 = t01 / l00, l20 = t02 / l00;   p1 = t11 - l10^2, l11 = sqrt(p1), l21 = (t12 - l20 l10) / l11;
//     p2 = t22 - l20^2 - l21^2, l22 = sqrt(p2);   w0 = d0 / l00, w1 = (d1 - l10 w0) / l11, w2 = (d2 - l20 w0 - l21 w1) / l22;
//     d2 = w0^2 + w1^2 + w2^2, logdet = ln p0 + ln p1 + ln p2                                  (k_calib's spelling for its S)
//     Li00 = 1 / l00, Li11 = 1 / l11, Li22 = 1 / l22, Li10 = -(l10 Li00) / l11, Li21 = -(l21 Li11) / l22, Li20 = -(l20 Li00 + l21 Li10) / l22;
//     ti00 = Li00^2 + Li10^2 + Li20^2, ti11 = Li11^2 + Li21^2, ti22 = Li22^2;   W_cc = 1 - n_c ti_cc
//     (C = 1: p0 = s + n, W = 1 - n / p0, d2 = d^2 / p0, logdet = ln p0)
//     q_mu = sum_c (mu_c - y_c)^2 - sum_c v^_c,     q_out = sum_c (out_c - y_c)^2 + sum_c (2 W_cc - 1) v^_c
// valid iff every input is finite and every pivot > 0; a degenerate pixel is counted and left out of everything else.  The inputs are built
// here: mu = net_out's first C planes, Sigma_x = U U^T or diag(a_c^2) with the products in fp64, n_c by head_sigma's rule on head_est's
// fp32 estimate (gauss: sig^2; poisson: max(mu_c, 1e-3) f), v^_c = n_c (gauss) or y_c f (poisson).  No 1e-6 regulariser.
// k_risk<C, DIAG>: one pixel per thread; the pixels of a sample's margin-shrunk region are numbered row-major n = (i - m) r2 + (j - m) and
//   workgroup k takes n = k * RB .. k * RB + RB - 1 (a function of (ext, margin) alone; loads stay coalesced along W).  The nine fp64 sums
//   go through a fixed shuffle tree per wave, then in wave order, the three counts as integers, all twelve into the workgroup's scratch slot.
// k_risk_final: one workgroup per sample adds the slots of its region's workgroups in a fixed order and writes stats[b].  Neither scratch
//   nor stats needs initial contents: a second launch, not a last-arriver ticket.
#pragma clang fp contract(off)
#include "head_math.h"
#include <cmath>

static constexpr int RB = SSDN_RISK_BLOCK, RS = SSDN_RISK_NSTATS;
static constexpr int RW = RB / 64;                             // waves of a block
// a workgroup's record in the order of stats[b]: 0, 1 and 11 are counts (unsigned 64-bit), 2..10 are fp64 sums
static constexpr int RD = 9, RC = 3;
static_assert(RS == RD + RC && RB % 64 == 0 && RB == HB, "a record is 9 sums and 3 counts");

// a sample's margin-shrunk region: r1 x r2 pixels from (margin, margin) of its extent, clamped to the tensor (ext is device memory)
static __device__ __forceinline__ void risk_region(const ssdn_risk_args& a, int b, int& r1, int& r2) {
    const int e1 = a.ext ? min(max(a.ext[2 * b], 0), a.H) : a.H;
    const int e2 = a.ext ? min(max(a.ext[2 * b + 1], 0), a.W) : a.W;
    const long long m2 = 2ll * a.margin;
    r1 = (int)max((long long)e1 - m2, 0ll);
    r2 = (int)max((long long)e2 - m2, 0ll);
}

template <int C, bool DIAG>
__global__ __launch_bounds__(RB) void k_risk(ssdn_risk_args a) {
    constexpr int NA = DIAG ? C : C * (C + 1) / 2, Cout = C + NA;
    __shared__ unsigned int cnt[RC];
    __shared__ double red[RD][RW];
    const int b = blockIdx.y;
    int r1, r2;
    risk_region(a, b, r1, r2);
    const long long n = (long long)r1 * r2;                     // (at most H * W: the launcher has bounded it)
    const long long first = (long long)blockIdx.x * RB;
    if (first >= n) return;                                     // (block-uniform: the workgroup lies outside the region)
    if (threadIdx.x < RC) cnt[threadIdx.x] = 0u;
    __syncthreads();
    const long long idx = first + threadIdx.x;
    const bool in = idx < n;
    const long long hw = (long long)a.H * a.W;
    bool valid = false;
    double v[RD];
#pragma unroll
    for (int k = 0; k < RD; ++k) v[k] = 0.0;
    unsigned int clip = 0;
    if (in) {
        const int i = (int)(idx / r2), j = (int)(idx - (long long)i * r2);
        const long long off = (long long)(i + a.margin) * a.W + (j + a.margin);
        const float* no = a.net_out + (long long)b * Cout * hw + off;
        const float est = head_est(a.mode, a.est_raw, b).est;
        const float npar = a.mode == 0 ? a.noise_param[b] : 0.f;
        const double f = a.mode == 0 ? 1.0 / (double)npar : (double)est;         // poisson: 1 / lambda or the estimate
        float muf[C], Af[NA];
        double mu[C], y[C], o[C], nc[C], vh[C];
        bool fin = true;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            muf[c] = no[c * hw];
            const float yf = a.noisy[((long long)b * C + c) * hw + off], of = a.pme[((long long)b * C + c) * hw + off];
            fin = fin && __builtin_isfinite(muf[c]) && __builtin_isfinite(yf) && __builtin_isfinite(of);
            mu[c] = (double)muf[c];
            y[c] = (double)yf;
            o[c] = (double)of;
        }
#pragma unroll
        for (int k = 0; k < NA; ++k) {
            Af[k] = no[(C + k) * hw];
            fin = fin && __builtin_isfinite(Af[k]);
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            if (a.style == 0) {
                const double sig = (double)head_sigma(0, a.mode, npar, est, muf[c]);
                nc[c] = sig * sig;
                vh[c] = nc[c];
            } else {
                nc[c] = (double)fmaxf(muf[c], 1e-3f) * f;
                vh[c] = y[c] * f;
            }
            fin = fin && __builtin_isfinite(nc[c]) && __builtin_isfinite(vh[c]);
            clip += (y[c] <= 0.0 || y[c] >= 1.0) ? 1u : 0u;
        }
        double d2, logdet, wcc[C];
        if constexpr (C == 3) {
            double s[6];                                         // Sigma_x, upper triangle 00, 01, 02, 11, 12, 22
            const double A0 = (double)Af[0], A1 = (double)Af[1], A2 = (double)Af[2];
            if constexpr (DIAG) {
                s[0] = A0 * A0; s[3] = A1 * A1; s[5] = A2 * A2;
                s[1] = s[2] = s[4] = 0.0;
            } else {                                             // U U^T, U = [[a0,a1,a2],[0,a3,a4],[0,0,a5]] (sym3_uut's sums)
                const double A3 = (double)Af[3], A4 = (double)Af[4], A5 = (double)Af[5];
                s[0] = (A0 * A0 + A1 * A1) + A2 * A2;
                s[1] = A1 * A3 + A2 * A4;
                s[2] = A2 * A5;
                s[3] = A3 * A3 + A4 * A4;
                s[4] = A4 * A5;
                s[5] = A5 * A5;
            }
            const double t00 = s[0] + nc[0], t01 = s[1], t02 = s[2], t11 = s[3] + nc[1], t12 = s[4], t22 = s[5] + nc[2];
            const double d0 = y[0] - mu[0], d1 = y[1] - mu[1], dd2 = y[2] - mu[2];
            const double p0 = t00, l00 = sqrt(p0), l10 = t01 / l00, l20 = t02 / l00;
            const double p1 = t11 - l10 * l10, l11 = sqrt(p1), l21 = (t12 - l20 * l10) / l11;
            const double p2 = (t22 - l20 * l20) - l21 * l21, l22 = sqrt(p2);
            const double w0 = d0 / l00, w1 = (d1 - l10 * w0) / l11, w2 = ((dd2 - l20 * w0) - l21 * w1) / l22;
            valid = fin && p0 > 0.0 && p1 > 0.0 && p2 > 0.0;
            d2 = (w0 * w0 + w1 * w1) + w2 * w2;
            logdet = (log(p0) + log(p1)) + log(p2);
            const double li00 = 1.0 / l00, li11 = 1.0 / l11, li22 = 1.0 / l22;
            const double li10 = -(l10 * li00) / l11;
            const double li21 = -(l21 * li11) / l22;
            const double li20 = -(l20 * li00 + l21 * li10) / l22;
            const double ti00 = (li00 * li00 + li10 * li10) + li20 * li20, ti11 = li11 * li11 + li21 * li21, ti22 = li22 * li22;
            wcc[0] = 1.0 - nc[0] * ti00;
            wcc[1] = 1.0 - nc[1] * ti11;
            wcc[2] = 1.0 - nc[2] * ti22;
        } else {
            const double A0 = (double)Af[0];
            const double p0 = A0 * A0 + nc[0], d0 = y[0] - mu[0];
            valid = fin && p0 > 0.0;
            d2 = (d0 * d0) / p0;
            logdet = log(p0);
            wcc[0] = 1.0 - nc[0] / p0;
        }
        if (valid) {
            double em = 0.0, eo = 0.0, sv = 0.0, sw = 0.0, trw = 0.0;
#pragma unroll
            for (int c = 0; c < C; ++c) {                        // (0.0 + x is x: the sums over c run left to right)
                const double a0 = mu[c] - y[c], b0 = o[c] - y[c];
                em = c ? em + a0 * a0 : a0 * a0;
                eo = c ? eo + b0 * b0 : b0 * b0;
                sv = c ? sv + vh[c] : vh[c];
                const double g = (2.0 * wcc[c] - 1.0) * vh[c];
                sw = c ? sw + g : g;
                trw = c ? trw + wcc[c] : wcc[c];
            }
            const double qm = em - sv, qo = eo + sw;
            v[0] = d2; v[1] = logdet; v[2] = em; v[3] = eo; v[4] = sv; v[5] = sw; v[6] = qm * qm; v[7] = qo * qo; v[8] = trw;
        } else clip = 0;
    }
    // the counts: ballots for the two pixel counts, a shuffle tree for the clipped pairs (at most 3 per lane); lane 0 adds to LDS
    const unsigned long long bv = __ballot(valid), bd = __ballot(in && !valid);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) clip += __shfl_down(clip, o, 64);
    // the sums: a shuffle tree per wave, then the waves in wave order
#pragma unroll
    for (int k = 0; k < RD; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_down(v[k], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&cnt[0], (unsigned int)__popcll(bv));
        atomicAdd(&cnt[1], (unsigned int)__popcll(bd));
        atomicAdd(&cnt[2], clip);
#pragma unroll
        for (int k = 0; k < RD; ++k) red[k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
    unsigned long long* slot = reinterpret_cast<unsigned long long*>(a.scratch) + ((long long)b * gridDim.x + blockIdx.x) * RS;
    if (threadIdx.x < RC) slot[threadIdx.x < 2 ? threadIdx.x : RS - 1] = cnt[threadIdx.x];
    if (threadIdx.x >= 64 && threadIdx.x < 64 + RD) {
        const int k = threadIdx.x - 64;
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < RW; ++w) t += red[k][w];
        reinterpret_cast<double*>(slot)[2 + k] = t;
    }
}

// stats[b]: the records of the sample's workgroups k = 0 .. ceil(r1 r2 / RB) - 1; thread t adds k = t, t + RB, ... in that order, then the
// block's fixed tree (the counts are integers until they are stored)
__global__ __launch_bounds__(RB) void k_risk_final(ssdn_risk_args a, int grid_blocks) {
    __shared__ double redd[RD][RW];
    __shared__ unsigned long long redu[RC][RW];
    const int b = blockIdx.x;
    int r1, r2;
    risk_region(a, b, r1, r2);
    const long long nblk = ((long long)r1 * r2 + RB - 1) / RB;
    const unsigned long long* part = reinterpret_cast<const unsigned long long*>(a.scratch) + (long long)b * grid_blocks * RS;
    double vd[RD];
    unsigned long long vu[RC] = {0, 0, 0};
#pragma unroll
    for (int m = 0; m < RD; ++m) vd[m] = 0.0;
    for (long long k = threadIdx.x; k < nblk; k += RB) {
        const unsigned long long* p = part + k * RS;
#pragma unroll
        for (int m = 0; m < RD; ++m) vd[m] += reinterpret_cast<const double*>(p)[2 + m];
#pragma unroll
        for (int m = 0; m < RC; ++m) vu[m] += p[m < 2 ? m : RS - 1];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int m = 0; m < RD; ++m) vd[m] += __shfl_down(vd[m], o, 64);
#pragma unroll
        for (int m = 0; m < RC; ++m) vu[m] += __shfl_down(vu[m], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int m = 0; m < RD; ++m) redd[m][threadIdx.x >> 6] = vd[m];
#pragma unroll
        for (int m = 0; m < RC; ++m) redu[m][threadIdx.x >> 6] = vu[m];
    }
    __syncthreads();
    double* out = a.stats + (long long)b * RS;
    if (threadIdx.x < RD) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < RW; ++w) t += redd[threadIdx.x][w];
        out[2 + threadIdx.x] = t;
    } else if (threadIdx.x >= 64 && threadIdx.x < 64 + RC) {
        const int m = threadIdx.x - 64;
        unsigned long long t = 0;
#pragma unroll
        for (int w = 0; w < RW; ++w) t += redu[m][w];
        out[m < 2 ? m : RS - 1] = (double)t;
    }
}

int launch_risk(const ssdn_risk_args* a, hipStream_t s) {
    if (!a->net_out || !a->noisy || !a->pme) return ssdn_set_error("risk: net_out, noisy and pme must be given");
    if (!a->stats) return ssdn_set_error("risk: the output stats must be given");
    if (a->C != 1 && a->C != 3) return ssdn_set_error("risk: C must be 1 or 3, got %d", a->C);
    if (a->B < 1 || a->H < 1 || a->W < 1) return ssdn_set_error("risk: B, H and W must be at least 1");
    if (a->margin < 0) return ssdn_set_error("risk: margin must be at least 0, got %d", a->margin);
    if (a->style == 2) return ssdn_set_error("risk: style 2 (impulse) is not supported: its posterior mean is not affine in the pixel and its noise is not zero-mean");
    if (a->style != 0 && a->style != 1) return ssdn_set_error("risk: style must be 0 (gauss) or 1 (poisson), got %d", a->style);
    if (a->mode < 0 || a->mode > 2) return ssdn_set_error("risk: mode must be 0, 1 or 2, got %d", a->mode);
    if (a->mode == 0 && !a->noise_param) return ssdn_set_error("risk: mode known needs noise_param");
    if (a->mode != 0 && !a->est_raw) return ssdn_set_error("risk: modes const / var need est_raw");
    if (a->diag != 0 && a->diag != 1) return ssdn_set_error("risk: diag must be 0 or 1, got %d", a->diag);
    if (!a->scratch) return ssdn_set_error("risk: scratch must be given");
    const long long hw = (long long)a->H * a->W;
    if (a->B > 65535 || hw > 2147483647LL - RB) return ssdn_set_error("risk: B must be at most 65535 and H * W at most 2^31 - 1 - %d", RB);
    if (a->scratch_bytes < SSDN_RISK_SCRATCH_BYTES((long long)a->B, a->C, a->H, a->W))
        return ssdn_set_error("risk: scratch_bytes is below SSDN_RISK_SCRATCH_BYTES(B, C, H, W)");
    if ((uintptr_t)a->scratch & 7) return ssdn_set_error("risk: scratch must be 8-byte aligned");
    const int blocks = (int)((hw + RB - 1) / RB);
    const dim3 grid((unsigned)blocks, (unsigned)a->B);
    if (a->C == 1) hipLaunchKernelGGL((k_risk<1, false>), grid, dim3(RB), 0, s, *a);         // (C = 1: the same model with or without diag)
    else if (a->diag) hipLaunchKernelGGL((k_risk<3, true>), grid, dim3(RB), 0, s, *a);
    else hipLaunchKernelGGL((k_risk<3, false>), grid, dim3(RB), 0, s, *a);
    hipLaunchKernelGGL(k_risk_final, dim3(a->B), dim3(RB), 0, s, *a, blocks);
    return 0;
}
