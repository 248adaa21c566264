// head_impulse.hip -- the loss head of the IMPULSE noise model (style 2; Laine et al.'s third corruption model), forward and
// vector-Jacobian product, fp32 (gfx950).  With probability alpha a pixel is replaced, in all channels, by a colour drawn uniformly
// from [0,1)^C; otherwise it is left alone.  Per pixel, with mu_x, Sigma_x = U U^T from net_out (sym3_uut) and e = mu_x - 1/2:
//   training loss: the Gaussian moment match of the mixture,
//     mu_y = alpha/2 + (1 - alpha) mu_x,   Sigma_y = (1 - alpha) Sigma_x + alpha/12 I + alpha (1 - alpha) e e^T   (a sum of PSD terms)
//     l = 1/2 log det Sigma_y + 1/2 d^T Sigma_y^-1 d,  d = y - mu_y   (C = 1: log sy + d^2 / sy);  l -= 0.1 alpha for a learnt alpha
//   posterior mean: the pixel is untouched (x = y) or replaced (x follows the prior),
//     Sigma_p = Sigma_x + 1e-6 I,  log f = log N(y; mu_x, Sigma_p),  w = sigmoid(log(1 - alpha) - log alpha + log f),  pme = mu_x + w (y - mu_x)
// Derivation, conditioning and measurements: DESIGN.md section 3.12.  Grid, pixel chunking (head_range), keep rule (head_vjp_kept) and
// partial[b][chunk][2] are k_head's, so k_head_final and k_fill_sigma_grad (head.hip) serve these kernels unchanged.  The symmetric 3x3
// helpers are head_math.h's.

// Every product and sum below is rounded on its own: whether the compiler fuses a multiply into an add depends on how many uses the
// product has, and g_net_out must not depend on whether g_noisy is requested (GY), bit for bit.  The kernels are HBM-bound.
// The pragma holds for the functions defined after it, head_math.h's included: it stays above the include.
#pragma clang fp contract(off)
#include "head_math.h"

// alpha as the head sees it and d alpha / d est_raw: known: clamp(noise_param, 1e-3, 0.999); const / var: the reference's softplus remap
// (denoiser.py:272-275) with an upper clamp, whose gradient is zero where it is active
struct ImpulseAlpha { float alpha, dalpha_draw, lodds, reg; };
static __device__ __forceinline__ ImpulseAlpha impulse_alpha(int mode, const float* noise_param, const float* est_raw, int b) {
    ImpulseAlpha r;
    r.dalpha_draw = 0.f;
    if (mode == 0) {
        r.alpha = fminf(fmaxf(noise_param[b], 1e-3f), 0.999f);
    } else {
        const float raw = est_raw[mode == 2 ? b : 0];
        const float sp = softplus_m4(raw);
        r.alpha = fminf(sp, 0.999f);
        r.dalpha_draw = sp < 0.999f ? sigmoid_m4(raw) : 0.f;
    }
    r.lodds = logf(1.f - r.alpha) - logf(r.alpha);
    r.reg = mode != 0 ? 0.1f : 0.f;
    return r;
}

// One pixel.  Reads mu, A (the C(C+1)/2 entries of U), y; sc = dL/dl of this pixel (LOSS weight over the pixel count), gp = dL/dpme.
//   do_loss: evaluate l (and, with do_grad, its gradient);  do_post: evaluate the posterior mean (and, with do_grad and gp, its gradient)
// Outputs: l, pme[C], and for do_grad g[Cout] = dL/dnet_out (without g_mu), gy[C] = the direct dL/dy, galpha = dL/dalpha.
template <int C> struct ImpulsePx {
    float l, pme[C], g[C + C * (C + 1) / 2], gy[C], galpha;
};
template <int C>
static __device__ __forceinline__ void impulse_px(const float* mu, const float* A, const float* y, const ImpulseAlpha& al, float sc,
                                                  const float* gp, bool do_loss, bool do_post, bool do_grad, ImpulsePx<C>& o) {
    const float alpha = al.alpha, om = 1.f - alpha, k = alpha * om;
    o.l = 0.f;
    o.galpha = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) { o.gy[c] = 0.f; o.pme[c] = 0.f; }
#pragma unroll
    for (int c = 0; c < C + C * (C + 1) / 2; ++c) o.g[c] = 0.f;
    if constexpr (C == 1) {
        const float a = A[0], sx = a * a, e = mu[0] - 0.5f;
        float gmu = 0.f, gx = 0.f;                          // dL/dmu_x, dL/dSigma_x
        if (do_loss) {
            const float sy = om * sx + alpha * (1.f / 12.f) + k * e * e;
            const float d = y[0] - (0.5f * alpha + om * mu[0]);
            const float rs = 1.f / sy, q = d * rs;
            o.l = logf(sy) + d * q - al.reg * alpha;
            if (do_grad) {
                const float G = sc * (rs - q * q);          // dL/dsy
                gmu = -2.f * sc * om * q + 2.f * k * G * e;
                gx = om * G;
                o.galpha = 2.f * sc * q * e + G * (1.f / 12.f - sx + (1.f - 2.f * alpha) * e * e) - al.reg * sc;
                o.gy[0] = 2.f * sc * q;
            }
        }
        if (do_post) {
            const float sp = sx + 1e-6f, r = y[0] - mu[0], rp = 1.f / sp, t = r * rp;
            const float z = al.lodds - 0.5f * logf(sp) - 0.5f * r * t - 0.9189385332f;
            const float w = 1.f / (1.f + expf(-z));
            o.pme[0] = mu[0] + w * r;
            if (do_grad && gp) {
                const float wm = 1.f / (1.f + expf(z));     // 1 - w without cancellation
                const float s = gp[0] * r * w * wm;         // dL/dz
                gmu += gp[0] * wm + s * t;
                gx += 0.5f * s * (t * t - rp);
                o.galpha -= s / k;
                o.gy[0] += gp[0] * w - s * t;
            }
        }
        o.g[0] = gmu;
        o.g[1] = 2.f * a * gx;
    } else {
        const Sym3 x = sym3_uut(A);
        const float e[3] = {mu[0] - 0.5f, mu[1] - 0.5f, mu[2] - 0.5f};
        float gmu[3] = {0.f, 0.f, 0.f};
        Sym3 gx = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};           // dL/dSigma_x as a symmetric matrix (k_head's convention: dL/dU = 2 G U)
        if (do_loss) {
            const float dg = alpha * (1.f / 12.f);
            Sym3 s, cf;
            s.m00 = om * x.m00 + dg + k * e[0] * e[0]; s.m01 = om * x.m01 + k * e[0] * e[1]; s.m02 = om * x.m02 + k * e[0] * e[2];
            s.m11 = om * x.m11 + dg + k * e[1] * e[1]; s.m12 = om * x.m12 + k * e[1] * e[2];
            s.m22 = om * x.m22 + dg + k * e[2] * e[2];
            const float det = sym3_adj(s, cf);              // Sigma_y >= alpha/12 I: det >= (1e-3 / 12)^3, no clamp
            const float rdet = 1.f / det;
            const float hm = 0.5f * alpha;
            const float d[3] = {y[0] - (hm + om * mu[0]), y[1] - (hm + om * mu[1]), y[2] - (hm + om * mu[2])};
            float q[3];
            sym3_mv(cf, d, rdet, q);
            o.l = 0.5f * logf(det) + 0.5f * (d[0] * q[0] + d[1] * q[1] + d[2] * q[2]) - al.reg * alpha;
            if (do_grad) {
                // G = dL/dSigma_y = sc/2 (Sy^-1 - q q^T), dL/dmu_y = -sc q
                const float hs = 0.5f * sc;
                Sym3 G;
                G.m00 = hs * (cf.m00 * rdet - q[0] * q[0]); G.m01 = hs * (cf.m01 * rdet - q[0] * q[1]); G.m02 = hs * (cf.m02 * rdet - q[0] * q[2]);
                G.m11 = hs * (cf.m11 * rdet - q[1] * q[1]); G.m12 = hs * (cf.m12 * rdet - q[1] * q[2]);
                G.m22 = hs * (cf.m22 * rdet - q[2] * q[2]);
                float Ge[3];
                sym3_mv(G, e, 1.f, Ge);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    gmu[c] = -sc * om * q[c] + 2.f * k * Ge[c];
                    o.gy[c] = sc * q[c];
                }
                gx = sym3_scale(G, om);
                const float gdotx = G.m00 * x.m00 + G.m11 * x.m11 + G.m22 * x.m22 + 2.f * (G.m01 * x.m01 + G.m02 * x.m02 + G.m12 * x.m12);
                const float tr = G.m00 + G.m11 + G.m22;
                const float eGe = e[0] * Ge[0] + e[1] * Ge[1] + e[2] * Ge[2];
                const float qe = q[0] * e[0] + q[1] * e[1] + q[2] * e[2];
                o.galpha = sc * qe + tr * (1.f / 12.f) - gdotx + (1.f - 2.f * alpha) * eGe - al.reg * sc;
            }
        }
        if (do_post) {
            const Sym3 sp = sym3_add_diag(x, 1e-6f, 1e-6f, 1e-6f);
            Sym3 cp;
            // exact arithmetic has det Sigma_p >= 1e-18 and a quadratic form >= 0; the fp32 adjugate of a rank-deficient Sigma_x may not
            const float detp = fmaxf(sym3_adj(sp, cp), 1e-18f);
            const float rdp = 1.f / detp;
            const float r[3] = {y[0] - mu[0], y[1] - mu[1], y[2] - mu[2]};
            float t[3];
            sym3_mv(cp, r, rdp, t);
            const float quad = fmaxf(r[0] * t[0] + r[1] * t[1] + r[2] * t[2], 0.f);
            const float z = al.lodds - 0.5f * logf(detp) - 0.5f * quad - 2.7568155996f;       // 3/2 log 2 pi
            const float w = 1.f / (1.f + expf(-z));
#pragma unroll
            for (int c = 0; c < 3; ++c) o.pme[c] = mu[c] + w * r[c];
            if (do_grad && gp) {
                const float wm = 1.f / (1.f + expf(z));     // 1 - w without cancellation
                const float s = (gp[0] * r[0] + gp[1] * r[1] + gp[2] * r[2]) * w * wm;       // dL/dz
                const float hs = 0.5f * s;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    gmu[c] += gp[c] * wm + s * t[c];
                    o.gy[c] += gp[c] * w - s * t[c];
                }
                // dL/dSigma_p = s/2 (t t^T - Sp^-1)
                gx.m00 += hs * (t[0] * t[0] - cp.m00 * rdp); gx.m01 += hs * (t[0] * t[1] - cp.m01 * rdp); gx.m02 += hs * (t[0] * t[2] - cp.m02 * rdp);
                gx.m11 += hs * (t[1] * t[1] - cp.m11 * rdp); gx.m12 += hs * (t[1] * t[2] - cp.m12 * rdp);
                gx.m22 += hs * (t[2] * t[2] - cp.m22 * rdp);
                o.galpha -= s / k;
            }
        }
        o.g[0] = gmu[0]; o.g[1] = gmu[1]; o.g[2] = gmu[2];
        sym3_dldu(gx, A, o.g + 3);
    }
}

template <int C>
__global__ __launch_bounds__(HB) void k_head_impulse(ssdn_head_args a) {
    __shared__ float sh[4];
    constexpr int NA = C * (C + 1) / 2, Cout = C + NA;
    const int b = blockIdx.y;
    const long long HW = (long long)a.H * a.W;
    const float inv_total = 1.f / ((float)a.B * (float)HW);  // mean over pixels, then mean over the batch
    const ImpulseAlpha al = impulse_alpha(a.mode, a.noise_param, a.est_raw, b);
    float loss_acc = 0.f, gal_acc = 0.f, gabs = 0.f;
    const HeadRange r = head_range(HW, a.nchunks);
    const float* no = a.net_out + (long long)b * Cout * HW;
    const float* ny = a.noisy + (long long)b * C * HW;
    for (long long p = r.p0 + threadIdx.x; p < r.p1; p += HB) {
        float mu[C], A[NA], y[C];
#pragma unroll
        for (int c = 0; c < C; ++c) { mu[c] = no[c * HW + p]; y[c] = ny[c * HW + p]; }
#pragma unroll
        for (int c = 0; c < NA; ++c) A[c] = no[(C + c) * HW + p];
        ImpulsePx<C> o;
        impulse_px<C>(mu, A, y, al, inv_total, nullptr, true, a.pme != nullptr, a.want_grad != 0, o);
        loss_acc += o.l;
        const long long oc = (long long)b * C * HW + p;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            if (a.mu) a.mu[oc + c * HW] = mu[c];
            if (a.pme) a.pme[oc + c * HW] = o.pme[c];
        }
        if (a.model_std) a.model_std[(long long)b * HW + p] = C == 1 ? fabsf(A[0]) : cbrtf(fabsf(A[0] * A[NA / 2] * A[NA - 1]));  // det(U U^T)^(1/2C)
        if (a.want_grad) {
#pragma unroll
            for (int c = 0; c < Cout; ++c) {
                a.g_net_out[((long long)b * Cout + c) * HW + p] = o.g[c];
                gabs = fmaxf(gabs, fabsf(o.g[c]));
            }
            gal_acc += o.galpha;
        }
    }
    const float ls = block_sum(loss_acc, sh);
    const float gs = block_sum(gal_acc, sh);
    if (threadIdx.x == 0) {
        float* pp = a.partial + ((long long)b * a.nchunks + blockIdx.x) * 2;
        pp[0] = ls;
        pp[1] = gs * al.dalpha_draw;
    }
    if (a.want_grad && a.gmax) atomic_max_abs_block(a.gmax, gabs, sh);
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.noise_std) a.noise_std[b] = al.alpha;       // NOISE_STD_DEV carries alpha, [B] like gauss
}

// Same grid, chunking and keep rule as k_head_vjp.  GY = (a.g_noisy != NULL): the direct term of dL/dnoisy, from the same pass (y enters
// d = y - mu_y, log f and w (y - mu_x)); a kept sample writes only that.
template <bool GY, int C>
__global__ __launch_bounds__(HB) void k_head_vjp_impulse(ssdn_head_vjp_args a) {
    __shared__ float sh[4];
    constexpr int NA = C * (C + 1) / 2, Cout = C + NA;
    const int b = blockIdx.y;
    const long long HW = (long long)a.H * a.W;
    const float wb = a.w ? a.w[b] : 0.f;
    const bool skip = head_vjp_kept(a.keep, a.g_pme, a.g_mu, a.w, wb, a.B);
    if (skip && !GY) return;                         // (block-uniform: before any barrier)
    const float sc = wb / (float)HW;        // LOSS[b] is the mean over the pixels of sample b
    const ImpulseAlpha al = impulse_alpha(a.mode, a.noise_param, a.est_raw, b);
    float gal_acc = 0.f, gabs = 0.f;
    const HeadRange r = head_range(HW, a.nchunks);
    const float* no = a.net_out + (long long)b * Cout * HW;
    const float* ny = a.noisy + (long long)b * C * HW;
    const float* gpp = a.g_pme ? a.g_pme + (long long)b * C * HW : nullptr;
    const float* gm = a.g_mu ? a.g_mu + (long long)b * C * HW : nullptr;
    float* go = a.g_net_out + (long long)b * Cout * HW;
    for (long long p = r.p0 + threadIdx.x; p < r.p1; p += HB) {
        float mu[C], A[NA], y[C], gp[C];
#pragma unroll
        for (int c = 0; c < C; ++c) { mu[c] = no[c * HW + p]; y[c] = ny[c * HW + p]; gp[c] = gpp ? gpp[c * HW + p] : 0.f; }
#pragma unroll
        for (int c = 0; c < NA; ++c) A[c] = no[(C + c) * HW + p];
        ImpulsePx<C> o;
        impulse_px<C>(mu, A, y, al, sc, gpp ? gp : nullptr, sc != 0.f, gpp != nullptr, true, o);
        if constexpr (GY) {
            float* gy = a.g_noisy + (long long)b * C * HW;
#pragma unroll
            for (int c = 0; c < C; ++c) gy[c * HW + p] = o.gy[c];
        }
        if (!skip) {
#pragma unroll
            for (int c = 0; c < Cout; ++c) {
                const float v = c < C && gm ? o.g[c] + gm[c * HW + p] : o.g[c];
                go[c * HW + p] = v;
                gabs = fmaxf(gabs, fabsf(v));
            }
            gal_acc += o.galpha;
        }
    }
    if (skip) return;                   // (block-uniform: the sample's g_net_out and partials stay the forward's)
    const float gs = block_sum(gal_acc, sh);
    if (threadIdx.x == 0) a.partial[((long long)b * a.nchunks + blockIdx.x) * 2 + 1] = gs * al.dalpha_draw;
    if (a.gmax) atomic_max_abs_block(a.gmax, gabs, sh);
}

// launch_head / launch_head_vjp (head.hip) have validated shape, style, mode and pointers
int launch_head_impulse(const ssdn_head_args* a, hipStream_t s) {
    if (a->diag) return ssdn_set_error("head: style 2 (impulse) with diag = 1 (DIAGONAL_COVARIANCE) is not supported");
    const dim3 grid(a->nchunks, a->B);
    if (a->C == 1) hipLaunchKernelGGL(k_head_impulse<1>, grid, dim3(HB), 0, s, *a);
    else hipLaunchKernelGGL(k_head_impulse<3>, grid, dim3(HB), 0, s, *a);
    return 0;
}
int launch_head_vjp_impulse(const ssdn_head_vjp_args* a, hipStream_t s) {
    if (a->diag) return ssdn_set_error("head_vjp: style 2 (impulse) with diag = 1 (DIAGONAL_COVARIANCE) is not supported");
    const dim3 grid(a->nchunks, a->B);
    if (a->C == 1) {
        if (a->g_noisy) hipLaunchKernelGGL((k_head_vjp_impulse<true, 1>), grid, dim3(HB), 0, s, *a);
        else hipLaunchKernelGGL((k_head_vjp_impulse<false, 1>), grid, dim3(HB), 0, s, *a);
    } else {
        if (a->g_noisy) hipLaunchKernelGGL((k_head_vjp_impulse<true, 3>), grid, dim3(HB), 0, s, *a);
        else hipLaunchKernelGGL((k_head_vjp_impulse<false, 3>), grid, dim3(HB), 0, s, *a);
    }
    return 0;
}
