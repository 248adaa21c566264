// head_posterior.hip -- SSDN_OP_HEAD_POSTERIOR: the per-pixel posterior the SSDN heads imply, beyond its mean: the covariance (upper
// triangle), the per-channel standard deviation and samples, fp32 (gfx950).  Nothing here is differentiable and no planned list holds it.
// Principle: Sigma_post is the matrix M for which the head's posterior mean is pme = M (Sx'^-1 mu + Sn'^-1 y), in the form that arm of
// k_head / k_head_impulse evaluates, so mean and covariance describe one Gaussian.  With Sigma_x = U U^T (sym3_uut), sigma_c (head_sigma),
// e = PME_EPS:
//   full, C = 3:  Sx' = Sigma_x + e I, Sn' = diag(sigma_c^2) + e I, T = Sx' + Sn', K = Sx' T^-1 (k_head's gain: pme = mu + K d);
//                 Sigma_post = sym(K Sn') = (Sx'^-1 + Sn'^-1)^-1.  The product form: Sx' - Sx' T^-1 Sx' cancels where the noise is small.
//   full, C = 1:  Sigma_post = sx sn / sy (no e, as in that arm's mean)
//   diagonal:     per channel rD_c = 1 / (ix_c + in_c + e), ix = 1/(sx + e), in = 1/(sn + e); off-diagonal entries 0
//   impulse:      the pixel is untouched (x = y) with probability w, or follows the prior: Sigma_post = (1 - w) Sigma_x + w (1 - w) r r^T,
//                 r = y - mu_x, w = k_head_impulse's sigmoid with its clamps
// Samples: x_s = pme + L z, L L^T = Sigma_post (Cholesky in registers, pivots clamped at 0); impulse: x_s = y exactly with probability w,
// else mu_x + U z.  Random numbers: philox.h, counter (b HW + p, PH_STREAM_POSTERIOR + 2 s + k, offset), key seed: sample s of a pixel
// is a pure function of (seed, offset, s, b, p), whatever n_samples and nchunks are.
// Derivation, conditioning and measurements: DESIGN.md section 3.13.  Grid (nchunks, B) and head_range are k_head's.  The few lines of
// head.hip / head_impulse.hip this file needs and those files keep to themselves (PME_EPS, the diagonal weights, alpha and the impulse
// weight) are restated here: the heads' generated code stays what it was.

// Every product and sum is rounded on its own, so that a value does not depend on which outputs were requested (head_impulse.hip's
// reason).  The pragma holds for the functions defined after it, head_math.h's included: it stays above the include.
#pragma clang fp contract(off)
#include "head_math.h"
#include "philox.h"

static constexpr float PP_EPS = 1e-6f;          // PME_EPS of head.hip

enum { PK_FULL1 = 0, PK_FULL3 = 1, PK_DIAG3 = 2, PK_IMP1 = 3, PK_IMP3 = 4 };

// log odds of "untouched" before the likelihood term: impulse_alpha of head_impulse.hip
static __device__ __forceinline__ float pp_impulse_lodds(int mode, const float* noise_param, const float* est_raw, int b) {
    float alpha;
    if (mode == 0) alpha = fminf(fmaxf(noise_param[b], 1e-3f), 0.999f);
    else alpha = fminf(softplus_m4(est_raw[mode == 2 ? b : 0]), 0.999f);
    return logf(1.f - alpha) - logf(alpha);
}

// lower Cholesky factor of a symmetric PSD 3x3 matrix, pivots clamped at 0 (a zero pivot zeroes its column)
struct Chol3 { float l00, l10, l20, l11, l21, l22; };
static __device__ __forceinline__ Chol3 chol3(const Sym3& s) {
    Chol3 l;
    l.l00 = sqrtf(fmaxf(s.m00, 0.f));
    const float r0 = l.l00 > 0.f ? 1.f / l.l00 : 0.f;
    l.l10 = s.m01 * r0;
    l.l20 = s.m02 * r0;
    l.l11 = sqrtf(fmaxf(s.m11 - l.l10 * l.l10, 0.f));
    const float r1 = l.l11 > 0.f ? 1.f / l.l11 : 0.f;
    l.l21 = (s.m12 - l.l20 * l.l10) * r1;
    l.l22 = sqrtf(fmaxf(s.m22 - l.l20 * l.l20 - l.l21 * l.l21, 0.f));
    return l;
}

template <int KIND, bool SAMP>
__global__ __launch_bounds__(HB) void k_head_posterior(ssdn_head_posterior_args a) {
    constexpr int C = (KIND == PK_FULL1 || KIND == PK_IMP1) ? 1 : 3;
    constexpr int NA = KIND == PK_DIAG3 ? 3 : C * (C + 1) / 2, Cout = C + NA, NT = C * (C + 1) / 2;
    constexpr bool IMP = KIND == PK_IMP1 || KIND == PK_IMP3;
    const int b = blockIdx.y;
    const long long HW = (long long)a.H * a.W;
    float est = 0.f, npar = 0.f, lodds = 0.f;
    if constexpr (IMP) lodds = pp_impulse_lodds(a.mode, a.noise_param, a.est_raw, b);
    else {
        est = head_est(a.mode, a.est_raw, b).est;
        npar = a.noise_param ? a.noise_param[b] : 0.f;
    }
    const HeadRange r = head_range(HW, a.nchunks);
    const float* no = a.net_out + (long long)b * Cout * HW;
    const float* ny = a.noisy + (long long)b * C * HW;
    float* cov = a.cov ? a.cov + (long long)b * NT * HW : nullptr;
    float* sd = a.std ? a.std + (long long)b * C * HW : nullptr;
    const unsigned k0 = (unsigned)a.seed, k1 = (unsigned)(a.seed >> 32), o0 = (unsigned)a.offset, o1 = (unsigned)(a.offset >> 32);
    for (long long p = r.p0 + threadIdx.x; p < r.p1; p += HB) {
        float mu[C], A[NA], y[C];
#pragma unroll
        for (int c = 0; c < C; ++c) { mu[c] = no[c * HW + p]; y[c] = ny[c * HW + p]; }
#pragma unroll
        for (int c = 0; c < NA; ++c) A[c] = no[(C + c) * HW + p];
        float cv[NT], ctr[C];              // Sigma_post (Sym3 order); the centre the Gaussian samples are drawn around
        float w = 0.f;                     // impulse: P(untouched | y)
        if constexpr (KIND == PK_FULL1) {
            float sig = head_sigma(a.style, a.mode, npar, est, mu[0]);
            const float sx = A[0] * A[0], sn = sig * sig, sy = sx + sn;
            cv[0] = sx * sn / sy;
            ctr[0] = (y[0] * sx + mu[0] * sn) / sy;
        } else if constexpr (KIND == PK_DIAG3) {
#pragma unroll
            for (int c = 0; c < NT; ++c) cv[c] = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float sig = head_sigma(a.style, a.mode, npar, est, mu[c]);
                const float ix = 1.f / (A[c] * A[c] + PP_EPS), in = 1.f / (sig * sig + PP_EPS);    // diag_pme_weights of head.hip
                const float rD = 1.f / (ix + in + PP_EPS);
                cv[c == 0 ? 0 : c == 1 ? 3 : 5] = rD;
                ctr[c] = mu[c] * (ix * rD) + y[c] * (in * rD);
            }
        } else if constexpr (KIND == PK_FULL3) {
            float n[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float sig = head_sigma(a.style, a.mode, npar, est, mu[c]);
                n[c] = sig * sig;
            }
            const Sym3 x = sym3_uut(A);
            const float e = PP_EPS;
            // T = (Sigma_x + Sigma_n) + 2 e I as k_head forms it; K = Sx' adj(T) / det T
            const Sym3 t = {(x.m00 + n[0]) + 2 * e, x.m01, x.m02, (x.m11 + n[1]) + 2 * e, x.m12, (x.m22 + n[2]) + 2 * e};
            Sym3 k;
            const float rd = 1.f / sym3_adj(t, k);
            const float d[3] = {y[0] - mu[0], y[1] - mu[1], y[2] - mu[2]};
            float q[3];
            sym3_mv(k, d, rd, q);
            const float xp0 = x.m00 + e, xp1 = x.m11 + e, xp2 = x.m22 + e;
            ctr[0] = mu[0] + xp0 * q[0] + x.m01 * q[1] + x.m02 * q[2];
            ctr[1] = mu[1] + x.m01 * q[0] + xp1 * q[1] + x.m12 * q[2];
            ctr[2] = mu[2] + x.m02 * q[0] + x.m12 * q[1] + xp2 * q[2];
            // G = Sx' adj(T): K = G / det T (not symmetric); Sigma_post = sym(K Sn'), (K Sn')_ij = K_ij n'_j
            const float g00 = xp0 * k.m00 + x.m01 * k.m01 + x.m02 * k.m02, g01 = xp0 * k.m01 + x.m01 * k.m11 + x.m02 * k.m12;
            const float g02 = xp0 * k.m02 + x.m01 * k.m12 + x.m02 * k.m22, g10 = x.m01 * k.m00 + xp1 * k.m01 + x.m12 * k.m02;
            const float g11 = x.m01 * k.m01 + xp1 * k.m11 + x.m12 * k.m12, g12 = x.m01 * k.m02 + xp1 * k.m12 + x.m12 * k.m22;
            const float g20 = x.m02 * k.m00 + x.m12 * k.m01 + xp2 * k.m02, g21 = x.m02 * k.m01 + x.m12 * k.m11 + xp2 * k.m12;
            const float g22 = x.m02 * k.m02 + x.m12 * k.m12 + xp2 * k.m22;
            const float m0 = (n[0] + e) * rd, m1 = (n[1] + e) * rd, m2 = (n[2] + e) * rd;
            cv[0] = g00 * m0;
            cv[1] = 0.5f * (g01 * m1 + g10 * m0);
            cv[2] = 0.5f * (g02 * m2 + g20 * m0);
            cv[3] = g11 * m1;
            cv[4] = 0.5f * (g12 * m2 + g21 * m1);
            cv[5] = g22 * m2;
        } else if constexpr (KIND == PK_IMP1) {
            // k_head_impulse's w (impulse_px, C = 1)
            const float sx = A[0] * A[0], sp = sx + 1e-6f, rr = y[0] - mu[0], t = rr * (1.f / sp);
            const float z = lodds - 0.5f * logf(sp) - 0.5f * rr * t - 0.9189385332f;
            w = 1.f / (1.f + expf(-z));
            const float wm = 1.f / (1.f + expf(z));
            cv[0] = wm * sx + (w * wm) * (rr * rr);
            ctr[0] = mu[0];
        } else {
            // k_head_impulse's w (impulse_px, C = 3)
            const Sym3 x = sym3_uut(A);
            const Sym3 sp = sym3_add_diag(x, 1e-6f, 1e-6f, 1e-6f);
            Sym3 cp;
            const float detp = fmaxf(sym3_adj(sp, cp), 1e-18f);
            const float rr[3] = {y[0] - mu[0], y[1] - mu[1], y[2] - mu[2]};
            float t[3];
            sym3_mv(cp, rr, 1.f / detp, t);
            const float quad = fmaxf(rr[0] * t[0] + rr[1] * t[1] + rr[2] * t[2], 0.f);
            const float z = lodds - 0.5f * logf(detp) - 0.5f * quad - 2.7568155996f;
            w = 1.f / (1.f + expf(-z));
            const float wm = 1.f / (1.f + expf(z)), ww = w * wm;
            cv[0] = wm * x.m00 + ww * (rr[0] * rr[0]); cv[1] = wm * x.m01 + ww * (rr[0] * rr[1]); cv[2] = wm * x.m02 + ww * (rr[0] * rr[2]);
            cv[3] = wm * x.m11 + ww * (rr[1] * rr[1]); cv[4] = wm * x.m12 + ww * (rr[1] * rr[2]);
            cv[5] = wm * x.m22 + ww * (rr[2] * rr[2]);
            ctr[0] = mu[0]; ctr[1] = mu[1]; ctr[2] = mu[2];
        }
        if (cov) {
#pragma unroll
            for (int c = 0; c < NT; ++c) cov[c * HW + p] = cv[c];
        }
        if (sd) {
#pragma unroll
            for (int c = 0; c < C; ++c) sd[c * HW + p] = sqrtf(fmaxf(cv[C == 1 ? 0 : c == 0 ? 0 : c == 1 ? 3 : 5], 0.f));
        }
        if constexpr (SAMP) {
            // the factor F of x_s = ctr + F z: lower triangular (Cholesky of Sigma_post), or for the impulse prior the upper triangular U
            float f[NT];
            if constexpr (C == 1) f[0] = IMP ? A[0] : sqrtf(fmaxf(cv[0], 0.f));
            else if constexpr (IMP) {
#pragma unroll
                for (int c = 0; c < 6; ++c) f[c] = A[c];
            } else if constexpr (KIND == PK_DIAG3) {
                f[0] = sqrtf(fmaxf(cv[0], 0.f)); f[3] = sqrtf(fmaxf(cv[3], 0.f)); f[5] = sqrtf(fmaxf(cv[5], 0.f));
                f[1] = f[2] = f[4] = 0.f;
            } else {
                const Chol3 l = chol3({cv[0], cv[1], cv[2], cv[3], cv[4], cv[5]});
                f[0] = l.l00; f[1] = l.l10; f[2] = l.l20; f[3] = l.l11; f[4] = l.l21; f[5] = l.l22;
            }
            const unsigned e0 = (unsigned)((long long)b * HW + p);
            float* sp = a.samples + (long long)b * C * HW + p;
            const long long sstride = (long long)a.B * C * HW;
            for (int s = 0; s < a.n_samples; ++s) {
                const Ph4 rn = philox4x32_10(e0, PH_STREAM_POSTERIOR + 2u * (unsigned)s, o0, o1, k0, k1);
                bool keep = false;
                if constexpr (IMP) {
                    const Ph4 ru = philox4x32_10(e0, PH_STREAM_POSTERIOR + 2u * (unsigned)s + 1u, o0, o1, k0, k1);
                    keep = u01(ru.v[0]) < w;
                }
                float v[C];
                if constexpr (C == 1) v[0] = ctr[0] + f[0] * ph_normal(rn.v[0], rn.v[1]);
                else {
                    float z0, z1;
                    ph_normal2(rn.v[0], rn.v[1], z0, z1);
                    const float z2 = ph_normal(rn.v[2], rn.v[3]);
                    if constexpr (IMP) {                 // U z
                        v[0] = ctr[0] + (f[0] * z0 + f[1] * z1 + f[2] * z2);
                        v[1] = ctr[1] + (f[3] * z1 + f[4] * z2);
                        v[2] = ctr[2] + f[5] * z2;
                    } else {                             // L z
                        v[0] = ctr[0] + f[0] * z0;
                        v[1] = ctr[1] + (f[1] * z0 + f[3] * z1);
                        v[2] = ctr[2] + (f[2] * z0 + f[4] * z1 + f[5] * z2);
                    }
                }
#pragma unroll
                for (int c = 0; c < C; ++c) sp[s * sstride + c * HW] = keep ? y[c] : v[c];
            }
        }
    }
}

// the argument rules of SSDN_OP_HEAD_POSTERIOR: check_head_args' (head.hip) for the fields the structs share, then the op's own; every
// one is decided on the host before any device call
static int check_posterior_args(const ssdn_head_posterior_args* a) {
    const char* op = "head_posterior";
    if (a->diag && a->C != 1 && a->C != 3) return ssdn_set_error("%s: diag needs C = 1 or 3", op);
    if (a->C != 1 && a->C != 3) return ssdn_set_error("%s: C must be 1 or 3 (denoiser.py:199)", op);
    if (a->diag != 0 && a->diag != 1) return ssdn_set_error("%s: diag must be 0 or 1", op);
    if (a->B < 1 || a->H < 1 || a->W < 1 || a->nchunks < 1) return ssdn_set_error("%s: bad shape", op);
    if (a->mode < 0 || a->mode > 2 || a->style < 0 || a->style > 2) return ssdn_set_error("%s: bad style / mode", op);
    if (!a->net_out || !a->noisy) return ssdn_set_error("%s: net_out and noisy must be given", op);
    if (!a->cov && !a->std && !a->samples) return ssdn_set_error("%s: one of cov, std and samples must be given", op);
    if (a->n_samples < 0 || (a->samples && a->n_samples < 1)) return ssdn_set_error("%s: samples needs n_samples >= 1", op);
    if (a->mode == 0 && !a->noise_param) return ssdn_set_error("%s: mode known needs noise_param", op);
    if (a->mode != 0 && !a->est_raw) return ssdn_set_error("%s: modes const / var need est_raw", op);
    if (a->style == 2 && a->diag) return ssdn_set_error("%s: style 2 (impulse) with diag = 1 (DIAGONAL_COVARIANCE) is not supported", op);
    // the random counter holds b HW + p in 32 bits and 2 s + 1 in 31
    if ((long long)a->B * a->H * a->W > 0xFFFFFFFFll) return ssdn_set_error("%s: B H W must be below 2^32", op);
    if (a->n_samples > (1 << 30)) return ssdn_set_error("%s: n_samples must be at most 2^30", op);
    return 0;
}

template <int KIND>
static void posterior_launch(const ssdn_head_posterior_args* a, hipStream_t s) {
    const dim3 grid(a->nchunks, a->B);
    if (a->samples) hipLaunchKernelGGL((k_head_posterior<KIND, true>), grid, dim3(HB), 0, s, *a);
    else hipLaunchKernelGGL((k_head_posterior<KIND, false>), grid, dim3(HB), 0, s, *a);
}

int launch_head_posterior(const ssdn_head_posterior_args* a, hipStream_t s) {
    if (int rc = check_posterior_args(a)) return rc;
    if (a->style == 2) {
        if (a->C == 1) posterior_launch<PK_IMP1>(a, s);
        else posterior_launch<PK_IMP3>(a, s);
    } else if (a->C == 1) posterior_launch<PK_FULL1>(a, s);         // (C = 1: the same model with or without diag, as in k_head)
    else if (a->diag) posterior_launch<PK_DIAG3>(a, s);
    else posterior_launch<PK_FULL3>(a, s);
    return 0;
}
