// head.hip -- per-pixel Gaussian posterior head + SSDN negative-log-likelihood, MSE and masked-MSE losses,
// forward AND hand-derived backward, fp32 (gfx950).  Replaces Denoiser._ssdn_pipeline / _mse_pipeline /
// _mask_mse_pipeline (/root/reference/ssdn/ssdn/denoiser.py:140-397, utils/n2v_loss.py:6-17) and their autograd graphs.
// The math (closed-form 3x3 SPD algebra and its derivative) is documented in DESIGN.md section "posterior head".
// The sigma rule, the softplus'd estimate, Sigma_x = U U^T, dL/dU = 2 G U, the pixel range and the keep rule are head_math.h's, shared
// with head_impulse.hip; so is the adjugate (sym3_adj) where it left the generated code alone: the posterior-mean terms of k_head_vjp
// and head_dy_pixel.
// k_head and k_head_vjp keep one arm per head kind (full C = 1, full C = 3, diagonal) inside their pixel loops, and four adjugates stay
// spelled out: this file is compiled with floating-point contraction on, and with the arms moved into per-pixel functions of their own
// (even word for word) or those adjugates routed through sym3_adj the compiler vectorised and contracted the arithmetic differently, or
// spilled more registers.  The kernels' results are kept bit for bit.
#include "head_math.h"

static constexpr float PME_EPS = 1e-6f;        // the reference's regulariser of the posterior mean's inverses
// ---- DIAGONAL_COVARIANCE: C = 3, net_out = [mu_0..2, a_0..2], Sigma_x = diag(a_c^2).  Every quantity is per
// channel: sy_c = a_c^2 + sigma_c^2, no adjugate.  (C = 1 is the same model with or without the flag: its runs use the DIAG = false code.)
// posterior mean of one channel, the reference's three eps-regularised inverses written for diagonal matrices:
//   pme = (mu ix + y in) / (ix + in + eps) = mu u + y v,   ix = 1/(sx + eps), in = 1/(sn + eps), u = ix rD, v = in rD, rD = 1/(ix + in + eps)
static __device__ __forceinline__ float diag_pme_weights(float sx, float sn, float& ix, float& in, float& u, float& v) {
    const float e = PME_EPS;
    ix = 1.f / (sx + e);
    in = 1.f / (sn + e);
    const float rD = 1.f / (ix + in + e);
    u = ix * rD;
    v = in * rD;
    return rD;
}

// posterior mean (denoiser.py:366-372) in its algebraically equal, well-conditioned form
//   (Sx'^-1 + Sn'^-1)^-1 (Sx'^-1 mu + Sn'^-1 y) = mu + Sx' T^-1 (y - mu),  Sx' = Sx + eps I, Sn' = Sn + eps I, T = Sx' + Sn' = Sy + 2 eps I
// adj T into k; returns 1 / det T
static __device__ __forceinline__ float gauss3_pme_adj(const Sym3& s, Sym3& k) {
    return 1.f / sym3_adj(sym3_add_diag(s, 2 * PME_EPS, 2 * PME_EPS, 2 * PME_EPS), k);
}
template <bool DIAG>
__global__ void k_head(ssdn_head_args a) {
    __shared__ float sh[4];
    const int b = blockIdx.y;
    const long long HW = (long long)a.H * a.W;
    const int C = a.C;
    const int Cout = DIAG ? 2 * C : C + C * (C + 1) / 2;
    const float inv_total = 1.f / ((float)a.B * (float)HW);  // mean over pixels, then mean over the batch
    const HeadEst he = head_est(a.mode, a.est_raw, b);
    const float est = he.est, dest_draw = he.dest_draw;
    const float npar = a.noise_param ? a.noise_param[b] : 0.f;
    float loss_acc = 0.f, gest_acc = 0.f, gabs = 0.f;
    const HeadRange r = head_range(HW, a.nchunks);
    const long long p0 = r.p0, p1 = r.p1;
    const float* no = a.net_out + (long long)b * Cout * HW;
    const float* ny = a.noisy + (long long)b * C * HW;
    for (long long p = p0 + threadIdx.x; p < p1; p += HB) {
        if constexpr (DIAG) {
            // l = 1/2 log(max(0, sy_0 sy_1 sy_2)) + 1/2 sum_c d_c^2 / sy_c  (- 0.1 mean_c sigma_c)
            float mu[3], av[3], sig[3], dsig_dmu[3], dsig_dest[3], sx[3], sn[3], rs[3], q[3];
            float prod = 1.f, quad = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                mu[c] = no[c * HW + p];
                av[c] = no[(3 + c) * HW + p];
                head_sigma(a.style, a.mode, npar, est, mu[c], sig[c], dsig_dmu[c], dsig_dest[c]);
                sx[c] = av[c] * av[c];
                sn[c] = sig[c] * sig[c];
                const float sy = sx[c] + sn[c], d = ny[c * HW + p] - mu[c];
                rs[c] = 1.f / sy;
                q[c] = d * rs[c];                                  // d_c / sy_c
                prod *= sy;
                quad += d * q[c];
            }
            float l = 0.5f * logf(fmaxf(prod, 0.f)) + 0.5f * quad;
            if (a.mode != 0) l -= 0.1f * (sig[0] + sig[1] + sig[2]) * (1.f / 3.f);
            loss_acc += l;
            long long o3 = (long long)b * 3 * HW + p;
            if (a.mu) { a.mu[o3] = mu[0]; a.mu[o3 + HW] = mu[1]; a.mu[o3 + 2 * HW] = mu[2]; }
            if (a.pme) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float ix, in, u, v;
                    diag_pme_weights(sx[c], sn[c], ix, in, u, v);
                    a.pme[o3 + c * HW] = mu[c] * u + ny[c * HW + p] * v;
                }
            }
            if (a.model_std) a.model_std[(long long)b * HW + p] = cbrtf(fabsf(av[0] * av[1] * av[2]));   // (prod sx_c)^(1/6)
            if (a.noise_std && a.style == 1) a.noise_std[(long long)b * HW + p] = cbrtf(sig[0] * sig[1] * sig[2]);
            if (a.want_grad) {
                // dl/dsy_c = 1/2 [prod > 0] / sy_c - 1/2 q_c^2; sx_c and sn_c enter through sy_c alone
                const float hd = prod > 0.f ? 0.5f : 0.f;
                const float reg = a.mode != 0 ? 0.1f / 3.f : 0.f;
                float gs = 0.f;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float gsy = hd * rs[c] - 0.5f * q[c] * q[c];
                    const float ds = 2.f * sig[c] * gsy - reg;
                    const float gmu = (-q[c] + ds * dsig_dmu[c]) * inv_total;
                    const float ga = 2.f * av[c] * gsy * inv_total;
                    a.g_net_out[((long long)b * 6 + c) * HW + p] = gmu;
                    a.g_net_out[((long long)b * 6 + 3 + c) * HW + p] = ga;
                    gabs = fmaxf(gabs, fmaxf(fabsf(gmu), fabsf(ga)));
                    gs += ds * dsig_dest[c];
                }
                gest_acc += gs;
            }
        } else if (C == 1) {
            float mu = no[p], av = no[HW + p], y = ny[p];
            float sig, dsig_dmu, dsig_dest;
            head_sigma(a.style, a.mode, npar, est, mu, sig, dsig_dmu, dsig_dest);
            float sx = av * av, sn = sig * sig, sy = sx + sn;
            float d = y - mu;
            float l = d * d / sy + logf(sy);
            if (a.mode != 0) l -= 0.1f * sig;
            loss_acc += l;
            if (a.mu) a.mu[(long long)b * HW + p] = mu;
            if (a.pme) a.pme[(long long)b * HW + p] = (y * sx + mu * sn) / sy;
            if (a.model_std) a.model_std[(long long)b * HW + p] = fabsf(av);
            if (a.noise_std && a.style == 1) a.noise_std[(long long)b * HW + p] = sig;
            if (a.want_grad) {
                float dsy = -d * d / (sy * sy) + 1.f / sy;
                float dsig = 2.f * sig * dsy - (a.mode != 0 ? 0.1f : 0.f);
                float gmu = (-2.f * d / sy + dsig * dsig_dmu) * inv_total;
                float ga = 2.f * av * dsy * inv_total;
                a.g_net_out[(long long)b * 2 * HW + p] = gmu;
                a.g_net_out[(long long)b * 2 * HW + HW + p] = ga;
                gabs = fmaxf(gabs, fmaxf(fabsf(gmu), fabsf(ga)));
                gest_acc += dsig * dsig_dest;
            }
        } else {
            float mu[3], A[6], y[3], sig[3], dsig_dmu[3], dsig_dest[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) { mu[c] = no[c * HW + p]; y[c] = ny[c * HW + p]; }
#pragma unroll
            for (int c = 0; c < 6; ++c) A[c] = no[(3 + c) * HW + p];
#pragma unroll
            for (int c = 0; c < 3; ++c) head_sigma(a.style, a.mode, npar, est, mu[c], sig[c], dsig_dmu[c], dsig_dest[c]);
            const Sym3 x = sym3_uut(A);
            const float x00 = x.m00, x01 = x.m01, x02 = x.m02, x11 = x.m11, x12 = x.m12, x22 = x.m22;
            float n0 = sig[0] * sig[0], n1 = sig[1] * sig[1], n2 = sig[2] * sig[2];
            float s00 = x00 + n0, s01 = x01, s02 = x02, s11 = x11 + n1, s12 = x12, s22 = x22 + n2;
            float d0 = y[0] - mu[0], d1 = y[1] - mu[1], d2 = y[2] - mu[2];
            // adjugate / determinant of the SPD 3x3 Sigma_y, here and for T below spelled out: through sym3_adj (head_math.h) this kernel
            // spilled two more VGPRs
            float c00 = s11 * s22 - s12 * s12, c01 = s02 * s12 - s01 * s22, c02 = s01 * s12 - s02 * s11;
            float c11 = s00 * s22 - s02 * s02, c12 = s01 * s02 - s00 * s12, c22 = s00 * s11 - s01 * s01;
            float det = s00 * c00 + s01 * c01 + s02 * c02;
            float rdet = 1.f / det;
            float i00 = c00 * rdet, i01 = c01 * rdet, i02 = c02 * rdet, i11 = c11 * rdet, i12 = c12 * rdet, i22 = c22 * rdet;
            float q0 = i00 * d0 + i01 * d1 + i02 * d2;
            float q1 = i01 * d0 + i11 * d1 + i12 * d2;
            float q2 = i02 * d0 + i12 * d1 + i22 * d2;
            float quad = d0 * q0 + d1 * q1 + d2 * q2;
            float detc = fmaxf(det, 0.f);
            float l = 0.5f * logf(detc) + 0.5f * quad;
            if (a.mode != 0) l -= 0.1f * (sig[0] + sig[1] + sig[2]) * (1.f / 3.f);
            loss_acc += l;
            long long o3 = (long long)b * 3 * HW + p;
            if (a.mu) { a.mu[o3] = mu[0]; a.mu[o3 + HW] = mu[1]; a.mu[o3 + 2 * HW] = mu[2]; }
            if (a.pme) {
                const float e = PME_EPS;
                float t00 = s00 + 2 * e, t11 = s11 + 2 * e, t22 = s22 + 2 * e;
                float k00 = t11 * t22 - s12 * s12, k01 = s02 * s12 - s01 * t22, k02 = s01 * s12 - s02 * t11;
                float k11 = t00 * t22 - s02 * s02, k12 = s01 * s02 - t00 * s12, k22 = t00 * t11 - s01 * s01;
                float rd = 1.f / (t00 * k00 + s01 * k01 + s02 * k02);
                float r0 = (k00 * d0 + k01 * d1 + k02 * d2) * rd;
                float r1 = (k01 * d0 + k11 * d1 + k12 * d2) * rd;
                float r2 = (k02 * d0 + k12 * d1 + k22 * d2) * rd;
                a.pme[o3] = mu[0] + (x00 + e) * r0 + x01 * r1 + x02 * r2;
                a.pme[o3 + HW] = mu[1] + x01 * r0 + (x11 + e) * r1 + x12 * r2;
                a.pme[o3 + 2 * HW] = mu[2] + x02 * r0 + x12 * r1 + (x22 + e) * r2;
            }
            if (a.model_std) a.model_std[(long long)b * HW + p] = cbrtf(fabsf(A[0] * A[3] * A[5]));  // det(U U^T)^(1/6)
            if (a.noise_std && a.style == 1) a.noise_std[(long long)b * HW + p] = cbrtf(sig[0] * sig[1] * sig[2]);
            if (a.want_grad) {
                // G = dl/dSigma_y = 1/2 Sy^-1 [det>0] - 1/2 q q^T
                float hd = det > 0.f ? 0.5f : 0.f;
                const Sym3 G = {hd * i00 - 0.5f * q0 * q0, hd * i01 - 0.5f * q0 * q1, hd * i02 - 0.5f * q0 * q2,
                                hd * i11 - 0.5f * q1 * q1, hd * i12 - 0.5f * q1 * q2, hd * i22 - 0.5f * q2 * q2};
                float reg = a.mode != 0 ? 0.1f / 3.f : 0.f;
                float ds0 = 2.f * sig[0] * G.m00 - reg, ds1 = 2.f * sig[1] * G.m11 - reg, ds2 = 2.f * sig[2] * G.m22 - reg;
                float g[9];
                g[0] = -q0 + ds0 * dsig_dmu[0];
                g[1] = -q1 + ds1 * dsig_dmu[1];
                g[2] = -q2 + ds2 * dsig_dmu[2];
                sym3_dldu(G, A, g + 3);
#pragma unroll
                for (int c = 0; c < 9; ++c) {
                    float v = g[c] * inv_total;
                    a.g_net_out[((long long)b * 9 + c) * HW + p] = v;
                    gabs = fmaxf(gabs, fabsf(v));
                }
                gest_acc += ds0 * dsig_dest[0] + ds1 * dsig_dest[1] + ds2 * dsig_dest[2];
            }
        }
    }
    float ls = block_sum(loss_acc, sh);
    float gs = block_sum(gest_acc, sh);
    if (threadIdx.x == 0) {
        float* pp = a.partial + ((long long)b * a.nchunks + blockIdx.x) * 2;
        pp[0] = ls;
        pp[1] = gs * dest_draw * inv_total;
    }
    if (a.want_grad && a.gmax) atomic_max_abs_block(a.gmax, gabs, sh);
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.noise_std && a.style == 0)
        a.noise_std[b] = head_sigma(0, a.mode, npar, est, 0.f);
}
// the argument rules of SSDN_OP_HEAD_SSDN and SSDN_OP_HEAD_VJP (the structs share these fields), every style; op: the error text's prefix
template <class Args>
static int check_head_args(const char* op, const Args* a, bool need_g) {
    if (a->diag && a->C != 1 && a->C != 3) return ssdn_set_error("%s: diag needs C = 1 or 3", op);
    if (a->C != 1 && a->C != 3) return ssdn_set_error("%s: C must be 1 or 3 (denoiser.py:199)", op);
    if (a->diag != 0 && a->diag != 1) return ssdn_set_error("%s: diag must be 0 or 1", op);
    if (a->B < 1 || a->H < 1 || a->W < 1 || a->nchunks < 1) return ssdn_set_error("%s: bad shape", op);
    if (a->mode < 0 || a->mode > 2 || a->style < 0 || a->style > 2) return ssdn_set_error("%s: bad style / mode", op);
    if (!a->net_out || !a->noisy || !a->partial) return ssdn_set_error("%s: net_out, noisy and partial must be given", op);
    if (need_g && !a->g_net_out) return ssdn_set_error("%s: g_net_out must be given", op);
    if (a->mode == 0 && !a->noise_param) return ssdn_set_error("%s: mode known needs noise_param", op);
    if (a->mode != 0 && !a->est_raw) return ssdn_set_error("%s: modes const / var need est_raw", op);
    return 0;
}
int launch_head(const ssdn_head_args* a, hipStream_t s) {
    if (int rc = check_head_args("head", a, a->want_grad != 0)) return rc;
    if (a->style == 2) return launch_head_impulse(a, s);          // head_impulse.hip
    if (a->diag && a->C == 3) hipLaunchKernelGGL(k_head<true>, dim3(a->nchunks, a->B), dim3(HB), 0, s, *a);
    else hipLaunchKernelGGL(k_head<false>, dim3(a->nchunks, a->B), dim3(HB), 0, s, *a);
    return 0;
}

// loss[b] (where asked for: the vector-Jacobian product passes loss = NULL) and g_est from the partials
__global__ void k_head_final(ssdn_head_final_args a) {
    // one thread per sample sums that sample's partials in index order (deterministic)
    int b = blockIdx.x * blockDim.x + threadIdx.x;
    long long HW = (long long)a.H * a.W;
    if (b < a.B) {
        float l = 0.f, g = 0.f;
        for (int c = 0; c < a.nchunks; ++c) {
            l += a.partial[((long long)b * a.nchunks + c) * 2];
            g += a.partial[((long long)b * a.nchunks + c) * 2 + 1];
        }
        if (a.loss) a.loss[b] = l / (float)HW;
        if (a.mode == 2 && a.g_est) a.g_est[b] = g;
    }
    if (a.mode == 1 && a.g_est && b == 0) {
        float g = 0.f;
        for (int bb = 0; bb < a.B; ++bb)
            for (int c = 0; c < a.nchunks; ++c) g += a.partial[((long long)bb * a.nchunks + c) * 2 + 1];
        a.g_est[0] = g;
    }
}
__global__ void k_fill_sigma_grad(ssdn_head_final_args a) {
    long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    long long HW = (long long)a.H * a.W;
    if (idx >= a.B * HW) return;
    int b = idx / HW;
    float v = a.g_est[b] / (float)HW;  // gradient of the spatial mean (denoiser.py:264)
    a.g_sigma_out[idx] = v;
    if ((idx % HW) == 0 && v != 0.f && a.gmax2) atomicMax(a.gmax2, __float_as_uint(fabsf(v)));
}
int launch_head_final(const ssdn_head_final_args* a, hipStream_t s) {
    hipLaunchKernelGGL(k_head_final, dim3((a->B + 63) / 64), dim3(64), 0, s, *a);
    if (a->mode == 2 && a->g_sigma_out) {
        long long n = (long long)a->B * a->H * a->W;
        hipLaunchKernelGGL(k_fill_sigma_grad, dim3((int)((n + 255) / 256)), dim3(256), 0, s, *a);
    }
    return 0;
}

__global__ void k_spatial_mean(ssdn_spatial_mean_args a) {
    __shared__ float sh[4];
    int b = blockIdx.x;
    float acc = 0.f;
    for (int i = threadIdx.x; i < a.HW; i += HB) acc += a.src[(long long)b * a.HW + i];
    float t = block_sum(acc, sh);
    if (threadIdx.x == 0) a.dst[b] = t / (float)a.HW;
}
int launch_spatial_mean(const ssdn_spatial_mean_args* a, hipStream_t s) {
    hipLaunchKernelGGL(k_spatial_mean, dim3(a->B), dim3(HB), 0, s, *a);
    return 0;
}

// MSE (denoiser.py:153-154): loss[b] = mean_{chw} (out-ref)^2 ; g = 2 (out-ref) / (CHW * B)
__global__ void k_mse(ssdn_mse_args a) {
    __shared__ float sh[4];
    int b = blockIdx.x;
    long long n = (long long)a.C * a.H * a.W;
    float acc = 0.f, gabs = 0.f;
    float k = 2.f / ((float)n * (float)a.B);
    for (long long i = threadIdx.x; i < n; i += HB) {
        float d = a.out[b * n + i] - a.ref[b * n + i];
        acc += d * d;
        if (a.g) {
            float g = k * d;
            a.g[b * n + i] = g;
            gabs = fmaxf(gabs, fabsf(g));
        }
    }
    float t = block_sum(acc, sh);
    if (threadIdx.x == 0) a.loss[b] = t / (float)n;
    if (a.g && a.gmax) atomic_max_abs(a.gmax, gabs);
}
// masked MSE (n2v_loss.py:6-17 + denoiser.py:175-176): coordinates of batch element 0 for every element, summed over
// coordinates, mean over channels.  Duplicate coordinates count twice (as in the reference's Python loop).
__global__ void k_mask_mse_zero(ssdn_mse_args a) {
    long long n = (long long)a.B * a.C * a.H * a.W;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) a.g[i] = 0.f;
}
__global__ void k_mask_mse(ssdn_mse_args a) {
    __shared__ float sh[4];
    int b = blockIdx.x;
    long long HW = (long long)a.H * a.W;
    float acc = 0.f;
    float k = 2.f / ((float)a.C * (float)a.B);
    // sequential over coordinates per (b,c) so that duplicate coordinates accumulate deterministically
    for (int c = threadIdx.x; c < a.C; c += HB) {
        for (int q = 0; q < a.ncoords; ++q) {
            long long r = a.coords[2 * q], cc = a.coords[2 * q + 1];
            if (r < 0 || r >= a.H || cc < 0 || cc >= a.W) continue;   // (the host validates; never touch memory outside the image)
            long long off = ((long long)b * a.C + c) * HW + r * a.W + cc;
            float d = a.out[off] - a.ref[off];
            acc += d * d;
            if (a.g) a.g[off] += k * d;
        }
    }
    float t = block_sum(acc, sh);
    if (threadIdx.x == 0) a.loss[b] = t / (float)a.C;
    if (a.g && a.gmax) {
        float gabs = 0.f;
        for (int c = threadIdx.x; c < a.C; c += HB)
            for (int q = 0; q < a.ncoords; ++q) {
                long long r = a.coords[2 * q], cc = a.coords[2 * q + 1];
                if (r < 0 || r >= a.H || cc < 0 || cc >= a.W) continue;
                gabs = fmaxf(gabs, fabsf(a.g[((long long)b * a.C + c) * HW + r * a.W + cc]));
            }
        atomic_max_abs(a.gmax, gabs);
    }
}
int launch_mse(const ssdn_mse_args* a, int masked, hipStream_t s) {
    if (!masked) {
        hipLaunchKernelGGL(k_mse, dim3(a->B), dim3(HB), 0, s, *a);
    } else {
        if (a->g) hipLaunchKernelGGL(k_mask_mse_zero, dim3(256), dim3(256), 0, s, *a);
        hipLaunchKernelGGL(k_mask_mse, dim3(a->B), dim3(HB), 0, s, *a);
    }
    return 0;
}

// H11 (SSDN_OP_METRICS): one block per sample; the block that arrives last adds the per-sample values in a fixed order
#define MB 1024          // threads of a k_metrics block: 16 waves (a sample is C*H*W = 12288 elements at BASELINE sizes: 12 per thread)
// the four per-sample sums of a block together: wave shuffle trees, one LDS slot per (wave, sum), every thread adds the 16 waves' values in
// wave order (two barriers for all four instead of two each)
static __device__ __forceinline__ void metrics_block_sum4(float (&v)[4], float (*sh)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_down(v[k], o, 64);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    if (l == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) sh[w][k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float t = 0.f;
#pragma unroll
        for (int j = 0; j < MB / 64; ++j) t += sh[j][k];
        v[k] = t;
    }
}
__global__ __launch_bounds__(MB) void k_metrics(ssdn_metrics_args a) {
    __shared__ float sh[MB / 64][4];
    __shared__ int last;
    const int b = blockIdx.x;
    const int HW = a.H * a.W;
    const int e1 = a.ext ? a.ext[2 * b] : a.H, e2 = a.ext ? a.ext[2 * b + 1] : a.W;
    const bool crop = e1 < a.H || e2 < a.W;      // (block-uniform: the coordinates of an element are only needed for a cropped extent)
    float so = 0.f, sm = 0.f, ss = 0.f, sn = 0.f;
    const long long base = (long long)b * a.C * HW;
    // (the trainer's kernel trace showed this launch at 50 us per step: 256 threads per sample, one element -- three loads and two
    //  integer divisions -- at a time.  Now 1024 threads with six elements' loads in flight each)
    constexpr int UNR = 6;
    const int n = a.C * HW;
    for (int i0 = threadIdx.x; i0 < n; i0 += MB * UNR) {
        float c[UNR], o[UNR], m[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int i = i0 + u * MB;
            bool ok = i < n;
            if (crop) {
                const int p = i % HW, y = p / a.W, x = p - y * a.W;
                ok = ok && y < e1 && x < e2;
            }
            c[u] = ok ? a.clean[base + i] : 0.f;
            o[u] = (ok && a.out) ? a.out[base + i] : c[u];
            m[u] = (ok && a.mu) ? a.mu[base + i] : c[u];
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const float d0 = o[u] - c[u], d1 = m[u] - c[u];
            so += d0 * d0;
            sm += d1 * d1;
        }
    }
    const bool npix = a.noise_std && a.noise_n == a.B * HW;
    for (int i0 = threadIdx.x; i0 < HW; i0 += MB * 4) {
        float v[4], w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * MB;
            v[u] = (a.model_std && i < HW) ? a.model_std[(long long)b * HW + i] : 0.f;
            w[u] = (npix && i < HW) ? a.noise_std[(long long)b * HW + i] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) { ss += v[u]; sn += w[u]; }
    }
    float sums[4] = {so, sm, ss, sn};
    metrics_block_sum4(sums, sh);
    so = sums[0]; sm = sums[1]; ss = sums[2]; sn = sums[3];
    if (threadIdx.x == 0) {
        const float cnt = (float)a.C * (float)e1 * (float)e2;
        float* q = a.per + 8 * b;
        q[0] = a.loss ? a.loss[b] : 0.f;
        q[1] = a.out ? -10.f * log10f(so / cnt) : 0.f;
        q[2] = a.mu ? -10.f * log10f(sm / cnt) : 0.f;
        q[3] = !a.noise_std ? 0.f : 255.f * (npix ? sn / (float)HW : a.noise_std[a.noise_n == a.B ? b : 0]);
        q[4] = a.model_std ? 255.f * ss / (float)HW : 0.f;
        __threadfence();
        const unsigned t = atomicAdd(reinterpret_cast<unsigned*>(a.acc + 15), 1u);
        last = t == (unsigned)a.B - 1;
    }
    __syncthreads();
    if (last && threadIdx.x < 64) {
        // the first wave of the last block: lane l fetches the five values of samples l, l + 64, ... (all loads independent -- one thread
        // per metric walking the samples was a chain of B dependent L2 round trips: 32 us at batch 32), then a fixed shuffle tree per metric
        __threadfence();
        const int l = threadIdx.x;
        float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        for (int j = l; j < a.B; j += 64) {
            float q[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) q[k] = __hip_atomic_load(a.per + 8 * j + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int k = 0; k < 5; ++k) v[k] += q[k];
        }
        const float first3 = __hip_atomic_load(a.per + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (sample 0's value: the metric of a batch with ONE noise level)
#pragma unroll
        for (int k = 0; k < 5; ++k)
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off);
        if (l == 0) {
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const bool on = k == 0 ? a.loss != nullptr : k == 1 ? a.out != nullptr : k == 2 ? a.mu != nullptr : k == 3 ? a.noise_std != nullptr : a.model_std != nullptr;
                if (!on) continue;
                const bool once = k == 3 && a.noise_n == 1;         // one noise level for the whole batch: a single sample of the metric
                a.acc[2 * k] += once ? first3 : v[k];
                a.acc[2 * k + 1] += once ? 1.f : (float)a.B;
            }
            *reinterpret_cast<unsigned*>(a.acc + 15) = 0u;
        }
    }
}
int launch_metrics(const ssdn_metrics_args* a, hipStream_t s) {
    if (!a->clean || !a->per || !a->acc) return ssdn_set_error("metrics: clean, per and acc must be given");
    if (a->B < 1 || a->C < 1 || a->H < 1 || a->W < 1) return ssdn_set_error("metrics: bad shape");
    if (a->noise_std && a->noise_n != 1 && a->noise_n != a->B && a->noise_n != a->B * a->H * a->W) return ssdn_set_error("metrics: noise_n must be 1, B or B*H*W");
    hipLaunchKernelGGL(k_metrics, dim3(a->B), dim3(MB), 0, s, *a);
    return 0;
}

// ---- SSDN_OP_HEAD_VJP / SSDN_OP_MSE_VJP: the pipelines' vector-Jacobian products for any upstream gradient ------------------------
// (Denoiser.run_pipeline under autograd: dL/dLOSS = w, dL/dIMG_DENOISED = g_pme, dL/dIMG_MU = g_mu; math in DESIGN.md section 3.8.)
// dL/dnoisy of the head at pixel p of one sample, net_out and sigma held fixed.  LOSS: C = 1, l = d^2/sy + log sy:
// 2 sc d/sy; C = 3, l = 1/2 d^T Sy^-1 d + 1/2 log det Sy: sc Sy^-1 d (adjugate over determinant).  Posterior mean: C = 1, (y sx + mu sn)/sy:
// g sx/sy; C = 3, mu + S' T^-1 d: h = T^-1 S' g.  IMG_MU does not read the noisy image.
static __device__ __forceinline__ void head_dy_pixel(const ssdn_head_vjp_args& a, const float* no, const float* ny, const float* gp, float* gy,
                                                     long long p, long long HW, float sc, float npar, float est) {
    if (a.C == 1) {
        float mu = no[p], av = no[HW + p], y = ny[p];
        float sig = head_sigma(a.style, a.mode, npar, est, mu);
        float sx = av * av, sy = sx + sig * sig, rs = 1.f / sy, d = y - mu;
        float v = sc != 0.f ? 2.f * d * rs * sc : 0.f;
        if (gp) v += gp[p] * sx * rs;
        gy[p] = v;
        return;
    }
    float A[6], mu[3], n[3];
#pragma unroll
    for (int c = 0; c < 6; ++c) A[c] = no[(3 + c) * HW + p];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        mu[c] = no[c * HW + p];
        float sig = head_sigma(a.style, a.mode, npar, est, mu[c]);
        n[c] = sig * sig;
    }
    const Sym3 x = sym3_uut(A);
    const float x00 = x.m00, x01 = x.m01, x02 = x.m02, x11 = x.m11, x12 = x.m12, x22 = x.m22;
    float s00 = x00 + n[0], s11 = x11 + n[1], s22 = x22 + n[2];
    float d0 = ny[p] - mu[0], d1 = ny[HW + p] - mu[1], d2 = ny[2 * HW + p] - mu[2];
    float v[3] = {0.f, 0.f, 0.f};
    if (sc != 0.f) {                    // sc Sy^-1 d (spelled out like the LOSS term of k_head_vjp's C = 3 arm, for the same reason)
        float c00 = s11 * s22 - x12 * x12, c01 = x02 * x12 - x01 * s22, c02 = x01 * x12 - x02 * s11;
        float c11 = s00 * s22 - x02 * x02, c12 = x01 * x02 - s00 * x12, c22 = s00 * s11 - x01 * x01;
        float rdet = 1.f / (s00 * c00 + x01 * c01 + x02 * c02);
        v[0] = (c00 * d0 + c01 * d1 + c02 * d2) * rdet * sc;
        v[1] = (c01 * d0 + c11 * d1 + c12 * d2) * rdet * sc;
        v[2] = (c02 * d0 + c12 * d1 + c22 * d2) * rdet * sc;
    }
    if (gp) {                           // h = T^-1 S' g, S' = Sx + eps I, T = Sy + 2 eps I
        const Sym3 s = {s00, x01, x02, s11, x12, s22};
        const float ga[3] = {gp[p], gp[HW + p], gp[2 * HW + p]};
        Sym3 k;
        float u[3], h[3];
        const float rd = gauss3_pme_adj(s, k);
        sym3_mv(sym3_add_diag(x, PME_EPS, PME_EPS, PME_EPS), ga, 1.f, u);
        sym3_mv(k, u, rd, h);
        v[0] += h[0]; v[1] += h[1]; v[2] += h[2];
    }
    gy[p] = v[0]; gy[HW + p] = v[1]; gy[2 * HW + p] = v[2];
}
// DIAG: per channel, LOSS sc d_c/sy_c, posterior mean g_c v_c (v_c = in_c / (ix_c + in_c + eps), diag_pme_weights)
static __device__ __forceinline__ void head_dy_pixel_diag(const ssdn_head_vjp_args& a, const float* no, const float* ny, const float* gp,
                                                          float* gy, long long p, long long HW, float sc, float npar, float est) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float mu = no[c * HW + p], av = no[(3 + c) * HW + p];
        float sig = head_sigma(a.style, a.mode, npar, est, mu);
        float sx = av * av, sn = sig * sig;
        float v = sc != 0.f ? (ny[c * HW + p] - mu) / (sx + sn) * sc : 0.f;
        if (gp) {
            float ix, in, u, w;
            diag_pme_weights(sx, sn, ix, in, u, w);
            v += gp[c * HW + p] * w;
        }
        gy[c * HW + p] = v;
    }
}
// Same grid and pixel chunking as k_head, so partial[b][chunk][1] lands where the forward put it.  A sample whose request is exactly
// the forward's d mean(LOSS) (keep, no g_pme / g_mu, w[b] == 1.f/B) leaves its gradient and partials alone, bit for bit: it returns at
// once, or, when g_noisy is requested, after writing only that.
// GY = (a.g_noisy != NULL): the head's direct term of dL/dnoisy in a second pass over the same pixels.  It re-reads
// its inputs instead of sharing the first pass's values: extra uses of those would let the compiler contract the g_net_out arithmetic
// differently, and the other outputs must not depend on GY, bit for bit.  The GY = true instance declares its real workgroup size (HB):
// under the default bound of 1024 threads (128 VGPRs) it spilled to scratch.
// DIAG: the diagonal-covariance head of k_head<true> (C = 3, Cout = 6), per-channel closed forms.
template <bool GY, bool DIAG>
__global__ __attribute__((amdgpu_flat_work_group_size(1, GY ? HB : 1024))) void k_head_vjp(ssdn_head_vjp_args a) {
    __shared__ float sh[4];
    const int b = blockIdx.y;
    const long long HW = (long long)a.H * a.W;
    const int C = a.C;
    const int Cout = DIAG ? 2 * C : C + C * (C + 1) / 2;
    const float wb = a.w ? a.w[b] : 0.f;
    const bool skip = head_vjp_kept(a.keep, a.g_pme, a.g_mu, a.w, wb, a.B);
    if (skip && !GY) return;                         // (block-uniform: before any barrier)
    const float sc = wb / (float)HW;        // LOSS[b] is the mean over the pixels of sample b
    const HeadEst he = head_est(a.mode, a.est_raw, b);
    const float est = he.est, dest_draw = he.dest_draw;
    const float npar = a.noise_param ? a.noise_param[b] : 0.f;
    const float reg = a.mode != 0 ? 0.1f : 0.f;
    float gest_acc = 0.f, gabs = 0.f;
    const HeadRange r = head_range(HW, a.nchunks);
    const long long p0 = r.p0, p1 = r.p1;
    const float* no = a.net_out + (long long)b * Cout * HW;
    const float* ny = a.noisy + (long long)b * C * HW;
    const float* gp = a.g_pme ? a.g_pme + (long long)b * C * HW : nullptr;
    const float* gm = a.g_mu ? a.g_mu + (long long)b * C * HW : nullptr;
    float* go = a.g_net_out + (long long)b * Cout * HW;
    const long long p1v = GY && skip ? p0 : p1;        // (a kept sample: no first pass)
    for (long long p = p0 + threadIdx.x; p < p1v; p += HB) {
        if constexpr (DIAG) {
            // per channel: dsx = dL/dsx_c, dn = dL/dsn_c, gmu = dL/dmu_c without the sigma chain
            float mu[3], av[3], y[3], sig[3], dsig_dmu[3], dsig_dest[3], sx[3], sn[3], dsx[3], dn[3], gmu[3];
            float prod = 1.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                mu[c] = no[c * HW + p];
                av[c] = no[(3 + c) * HW + p];
                y[c] = ny[c * HW + p];
                head_sigma(a.style, a.mode, npar, est, mu[c], sig[c], dsig_dmu[c], dsig_dest[c]);
                sx[c] = av[c] * av[c];
                sn[c] = sig[c] * sig[c];
                prod *= sx[c] + sn[c];
                dsx[c] = dn[c] = gmu[c] = 0.f;
            }
            float rg = 0.f;
            if (sc != 0.f) {            // LOSS: dl/dsy_c = 1/2 [prod > 0] / sy_c - 1/2 q_c^2, dl/dmu_c = -q_c, q_c = d_c / sy_c
                const float hd = prod > 0.f ? 0.5f : 0.f;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float rs = 1.f / (sx[c] + sn[c]), q = (y[c] - mu[c]) * rs;
                    dsx[c] = dn[c] = (hd * rs - 0.5f * q * q) * sc;
                    gmu[c] = -q * sc;
                }
                rg = reg * (1.f / 3.f) * sc;
            }
            if (gp) {                   // posterior mean mu u + y v: d/dmu = u, d/dsx = (pme - mu) ix u, d/dsn = (pme - y) in v
                const float e = 1e-6f;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float ix, in, u, v;
                    const float re = e * diag_pme_weights(sx[c], sn[c], ix, in, u, v);        // eps rD
                    const float g = gp[c * HW + p], d = y[c] - mu[c];
                    gmu[c] += g * u;
                    dsx[c] += g * (d * v - mu[c] * re) * ix * u;            // pme - mu = d v - mu eps rD (no cancellation)
                    dn[c] -= g * (d * u + y[c] * re) * in * v;              // pme - y = -(d u + y eps rD)
                }
            }
            float gs = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float ds = 2.f * sig[c] * dn[c] - rg;
                const float gm_c = gmu[c] + ds * dsig_dmu[c] + (gm ? gm[c * HW + p] : 0.f);
                const float ga = 2.f * av[c] * dsx[c];
                go[c * HW + p] = gm_c;
                go[(3 + c) * HW + p] = ga;
                gabs = fmaxf(gabs, fmaxf(fabsf(gm_c), fabsf(ga)));
                gs += ds * dsig_dest[c];
            }
            gest_acc += gs;
        } else if (C == 1) {
            float mu = no[p], av = no[HW + p], y = ny[p];
            float sig, dsig_dmu, dsig_dest;
            head_sigma(a.style, a.mode, npar, est, mu, sig, dsig_dmu, dsig_dest);
            float sx = av * av, sn = sig * sig, sy = sx + sn;
            float d = y - mu;
            float dmu = 0.f, dsx = 0.f, dsn = 0.f, dsig = 0.f;
            if (sc != 0.f) {            // LOSS: l = d^2/sy + log sy (- 0.1 sig)
                float dsy = (-d * d / (sy * sy) + 1.f / sy) * sc;
                dmu = -2.f * d / sy * sc;
                dsx = dsy;
                dsn = dsy;
                dsig = -reg * sc;
            }
            if (gp) {                   // posterior mean (y sx + mu sn) / sy
                float g = gp[p], rs = 1.f / sy;
                float t = g * d * rs * rs;
                dmu += g * sn * rs;
                dsx += sn * t;
                dsn -= sx * t;
            }
            dsig += 2.f * sig * dsn;
            float gmu = dmu + dsig * dsig_dmu + (gm ? gm[p] : 0.f);
            float ga = 2.f * av * dsx;
            go[p] = gmu;
            go[HW + p] = ga;
            gabs = fmaxf(gabs, fmaxf(fabsf(gmu), fabsf(ga)));
            gest_acc += dsig * dsig_dest;
        } else {
            float mu[3], A[6], y[3], sig[3], dsig_dmu[3], dsig_dest[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) { mu[c] = no[c * HW + p]; y[c] = ny[c * HW + p]; }
#pragma unroll
            for (int c = 0; c < 6; ++c) A[c] = no[(3 + c) * HW + p];
#pragma unroll
            for (int c = 0; c < 3; ++c) head_sigma(a.style, a.mode, npar, est, mu[c], sig[c], dsig_dmu[c], dsig_dest[c]);
            const Sym3 x = sym3_uut(A);
            const Sym3 s = sym3_add_diag(x, sig[0] * sig[0], sig[1] * sig[1], sig[2] * sig[2]);
            const float d[3] = {y[0] - mu[0], y[1] - mu[1], y[2] - mu[2]};
            const float x00 = x.m00, x01 = x.m01, x02 = x.m02, x11 = x.m11, x12 = x.m12, x22 = x.m22;
            const float s00 = s.m00, s01 = s.m01, s02 = s.m02, s11 = s.m11, s12 = s.m12, s22 = s.m22;
            const float d0 = d[0], d1 = d[1], d2 = d[2];
            // G: dL/dSigma_x as a symmetric matrix (dL/dx01 as a scalar = 2 G01, the convention of sym3_dldu);
            // dn: dL/d(sigma_c^2); gmu: dL/dmu without the sigma chain
            float g00 = 0.f, g01 = 0.f, g02 = 0.f, g11 = 0.f, g12 = 0.f, g22 = 0.f;
            float dn0 = 0.f, dn1 = 0.f, dn2 = 0.f, gmu0 = 0.f, gmu1 = 0.f, gmu2 = 0.f, rg = 0.f;
            if (sc != 0.f) {            // LOSS: 1/2 log det Sy + 1/2 d^T Sy^-1 d (- 0.1 mean sig); G = 1/2 Sy^-1 [det>0] - 1/2 q q^T
                // (this adjugate stays spelled out: through sym3_adj the compiler contracted this kernel's arithmetic differently)
                float c00 = s11 * s22 - s12 * s12, c01 = s02 * s12 - s01 * s22, c02 = s01 * s12 - s02 * s11;
                float c11 = s00 * s22 - s02 * s02, c12 = s01 * s02 - s00 * s12, c22 = s00 * s11 - s01 * s01;
                float det = s00 * c00 + s01 * c01 + s02 * c02;
                float rdet = 1.f / det;
                float i00 = c00 * rdet, i01 = c01 * rdet, i02 = c02 * rdet, i11 = c11 * rdet, i12 = c12 * rdet, i22 = c22 * rdet;
                float q0 = i00 * d0 + i01 * d1 + i02 * d2;
                float q1 = i01 * d0 + i11 * d1 + i12 * d2;
                float q2 = i02 * d0 + i12 * d1 + i22 * d2;
                float hd = det > 0.f ? 0.5f : 0.f;
                g00 = (hd * i00 - 0.5f * q0 * q0) * sc; g01 = (hd * i01 - 0.5f * q0 * q1) * sc; g02 = (hd * i02 - 0.5f * q0 * q2) * sc;
                g11 = (hd * i11 - 0.5f * q1 * q1) * sc; g12 = (hd * i12 - 0.5f * q1 * q2) * sc; g22 = (hd * i22 - 0.5f * q2 * q2) * sc;
                dn0 = g00; dn1 = g11; dn2 = g22;
                gmu0 = -q0 * sc; gmu1 = -q1 * sc; gmu2 = -q2 * sc;
                rg = reg * (1.f / 3.f) * sc;
            }
            if (gp) {                   // posterior mean mu + S' T^-1 d, S' = Sx + eps I, T = Sy + 2 eps I (the forward's form)
                const float e = PME_EPS;
                float ga0 = gp[p], ga1 = gp[HW + p], ga2 = gp[2 * HW + p];
                Sym3 kk;
                float rd = gauss3_pme_adj(s, kk);
                const float k00 = kk.m00, k01 = kk.m01, k02 = kk.m02, k11 = kk.m11, k12 = kk.m12, k22 = kk.m22;
                float r0 = (k00 * d0 + k01 * d1 + k02 * d2) * rd;
                float r1 = (k01 * d0 + k11 * d1 + k12 * d2) * rd;
                float r2 = (k02 * d0 + k12 * d1 + k22 * d2) * rd;
                float u0 = (x00 + e) * ga0 + x01 * ga1 + x02 * ga2;       // S' g
                float u1 = x01 * ga0 + (x11 + e) * ga1 + x12 * ga2;
                float u2 = x02 * ga0 + x12 * ga1 + (x22 + e) * ga2;
                float h0 = (k00 * u0 + k01 * u1 + k02 * u2) * rd;        // h = T^-1 S' g
                float h1 = (k01 * u0 + k11 * u1 + k12 * u2) * rd;
                float h2 = (k02 * u0 + k12 * u1 + k22 * u2) * rd;
                float e0 = ga0 - h0, e1 = ga1 - h1, e2 = ga2 - h2;
                gmu0 += e0; gmu1 += e1; gmu2 += e2;
                g00 += e0 * r0; g11 += e1 * r1; g22 += e2 * r2;          // (g - h) r^T, symmetrised
                g01 += 0.5f * (e0 * r1 + e1 * r0);
                g02 += 0.5f * (e0 * r2 + e2 * r0);
                g12 += 0.5f * (e1 * r2 + e2 * r1);
                dn0 -= h0 * r0; dn1 -= h1 * r1; dn2 -= h2 * r2;
            }
            float ds0 = 2.f * sig[0] * dn0 - rg, ds1 = 2.f * sig[1] * dn1 - rg, ds2 = 2.f * sig[2] * dn2 - rg;
            float g[9];
            g[0] = gmu0 + ds0 * dsig_dmu[0] + (gm ? gm[p] : 0.f);
            g[1] = gmu1 + ds1 * dsig_dmu[1] + (gm ? gm[HW + p] : 0.f);
            g[2] = gmu2 + ds2 * dsig_dmu[2] + (gm ? gm[2 * HW + p] : 0.f);
            { const Sym3 G = {g00, g01, g02, g11, g12, g22}; sym3_dldu(G, A, g + 3); }
#pragma unroll
            for (int c = 0; c < 9; ++c) {
                go[c * HW + p] = g[c];
                gabs = fmaxf(gabs, fabsf(g[c]));
            }
            gest_acc += ds0 * dsig_dest[0] + ds1 * dsig_dest[1] + ds2 * dsig_dest[2];
        }
    }
    if constexpr (GY) {
        float* gy = a.g_noisy + (long long)b * C * HW;
        for (long long p = p0 + threadIdx.x; p < p1; p += HB) {
            if constexpr (DIAG) head_dy_pixel_diag(a, no, ny, gp, gy, p, HW, sc, npar, est);
            else head_dy_pixel(a, no, ny, gp, gy, p, HW, sc, npar, est);
        }
        if (skip) return;               // (block-uniform: the sample's g_net_out and partials stay the forward's)
    }
    float gs = block_sum(gest_acc, sh);
    if (threadIdx.x == 0) a.partial[((long long)b * a.nchunks + blockIdx.x) * 2 + 1] = gs * dest_draw;
    if (a.gmax) atomic_max_abs_block(a.gmax, gabs, sh);
}
int launch_head_vjp(const ssdn_head_vjp_args* a, hipStream_t s) {
    if (int rc = check_head_args("head_vjp", a, true)) return rc;
    const dim3 grid(a->nchunks, a->B);
    if (a->style == 2) {                                             // head_impulse.hip; the reductions below serve it unchanged
        if (int rc = launch_head_vjp_impulse(a, s)) return rc;
    } else if (a->diag && a->C == 3) {
        if (a->g_noisy) hipLaunchKernelGGL((k_head_vjp<true, true>), grid, dim3(HB), 0, s, *a);
        else hipLaunchKernelGGL((k_head_vjp<false, true>), grid, dim3(HB), 0, s, *a);
    } else if (a->g_noisy) hipLaunchKernelGGL((k_head_vjp<true, false>), grid, dim3(HB), 0, s, *a);
    else hipLaunchKernelGGL((k_head_vjp<false, false>), grid, dim3(HB), 0, s, *a);
    if (a->mode != 0 && a->g_est) {
        // g_est from the partials in the forward's order (kept samples' partials are the forward's: the sum is too); no loss store
        const ssdn_head_final_args f = {a->partial, a->B, a->nchunks, a->H, a->W, a->mode, nullptr, a->g_est, a->g_sigma_out, a->gmax2};
        return launch_head_final(&f, s);
    }
    return 0;
}

// g = w[b] dLOSS[b]/dout + g_pme, one block per sample.  MSE: LOSS[b] = mean_chw (out - ref)^2.  Masked: g_pme everywhere, then the
// loss term added at element 0's coordinates, channel-sequential over the coordinates as in k_mask_mse (duplicates count twice).
__global__ void k_mse_vjp(ssdn_mse_vjp_args a) {
    __shared__ float sh[4];
    const int b = blockIdx.x;
    const long long HW = (long long)a.H * a.W;
    const long long n = (long long)a.C * HW;
    const float wb = a.w ? a.w[b] : 0.f;
    if (a.keep && !a.g_pme && a.w && wb == 1.f / (float)a.B) return;             // (block-uniform: before any barrier)
    float* g = a.g + b * n;
    const float* gp = a.g_pme ? a.g_pme + b * n : nullptr;
    const float* out = a.out + b * n;
    const float* ref = a.ref ? a.ref + b * n : nullptr;
    const bool lossg = a.w && ref;
    float gabs = 0.f;
    if (!a.masked) {
        const float k = wb * (2.f / (float)n);
        for (long long i = threadIdx.x; i < n; i += HB) {
            float v = lossg ? k * (out[i] - ref[i]) : 0.f;
            if (gp) v += gp[i];
            g[i] = v;
            gabs = fmaxf(gabs, fabsf(v));
        }
    } else {
        for (long long i = threadIdx.x; i < n; i += HB) g[i] = gp ? gp[i] : 0.f;
        __syncthreads();
        if (lossg && a.coords) {
            const float k = wb * (2.f / (float)a.C);
            for (int c = threadIdx.x; c < a.C; c += HB)
                for (int q = 0; q < a.ncoords; ++q) {
                    long long r = a.coords[2 * q], cc = a.coords[2 * q + 1];
                    if (r < 0 || r >= a.H || cc < 0 || cc >= a.W) continue;
                    long long off = c * HW + r * a.W + cc;
                    g[off] += k * (out[off] - ref[off]);
                }
        }
        __syncthreads();
        for (long long i = threadIdx.x; i < n; i += HB) gabs = fmaxf(gabs, fabsf(g[i]));
    }
    if (a.gmax) atomic_max_abs_block(a.gmax, gabs, sh);
}
int launch_mse_vjp(const ssdn_mse_vjp_args* a, hipStream_t s) {
    if (a->B < 1 || a->C < 1 || a->H < 1 || a->W < 1) return ssdn_set_error("mse_vjp: bad shape");
    if (!a->out || !a->g) return ssdn_set_error("mse_vjp: out and g must be given");
    if (a->w && !a->ref) return ssdn_set_error("mse_vjp: a LOSS gradient needs ref");
    if (a->w && a->masked && (!a->coords || a->ncoords < 0)) return ssdn_set_error("mse_vjp: masked LOSS gradient needs coords");
    hipLaunchKernelGGL(k_mse_vjp, dim3(a->B), dim3(HB), 0, s, *a);
    return 0;
}
