// head_math.h -- the per-pixel algebra the loss heads share, each piece written once (head.hip: full and diagonal Gaussian / Poisson heads;
// head_impulse.hip: the impulse head): the noise-sigma rule, the softplus'd noise estimate, symmetric 3x3 helpers (Sigma_x = U U^T,
// adjugate and determinant, matrix-vector product, dL/dU = 2 G U), a block's pixel range and the keep rule of the vector-Jacobian product.
// Everything is __forceinline__ and takes the caller's locals, so a kernel's arithmetic is what it was when it spelled these out by hand.
// A file that wants its products and sums rounded one by one puts "#pragma clang fp contract(off)" ABOVE this include: the pragma holds
// for the functions defined after it.
#pragma once
#include "head_common.h"

// sigma_c of one channel, and its derivatives by mu_c and by the softplus'd estimate.  style 0 (gauss): the known sigma (floored) or the
// estimate; style 1 (poisson): sqrt(max(mu, 1e-3) f), f = 1 / lambda or the estimate.  A caller that needs sig alone drops the other two.
static __device__ __forceinline__ void head_sigma(int style, int mode, float npar, float est, float mu, float& sig, float& dsig_dmu,
                                                  float& dsig_dest) {
    if (style == 0) {
        sig = mode == 0 ? fmaxf(npar, 1e-3f) : est;
        dsig_dmu = 0.f;
        dsig_dest = 1.f;
    } else {
        float m = fmaxf(mu, 1e-3f);
        float f = mode == 0 ? 1.f / npar : est;
        sig = sqrtf(m * f);
        dsig_dmu = mu > 1e-3f ? 0.5f * f / sig : 0.f;
        dsig_dest = 0.5f * m / sig;
    }
}
static __device__ __forceinline__ float head_sigma(int style, int mode, float npar, float est, float mu) {
    float sig, dsig_dmu, dsig_dest;
    head_sigma(style, mode, npar, est, mu, sig, dsig_dmu, dsig_dest);
    return sig;
}

// the learnt noise estimate of sample b as the heads see it (the reference's softplus remap) and its derivative by the raw value;
// mode known: none
struct HeadEst { float est, dest_draw; };
static __device__ __forceinline__ HeadEst head_est(int mode, const float* est_raw, int b) {
    HeadEst r = {0.f, 0.f};
    if (mode != 0) {
        float raw = est_raw[mode == 2 ? b : 0];
        r.est = softplus_m4(raw);
        r.dest_draw = sigmoid_m4(raw);
    }
    return r;
}

// the pixels [p0, p1) of block blockIdx.x among the nchunks blocks of a sample (the last one may get fewer)
struct HeadRange { long long p0, p1; };
static __device__ __forceinline__ HeadRange head_range(long long HW, int nchunks) {
    const long long per = (HW + nchunks - 1) / nchunks;
    const long long p0 = (long long)blockIdx.x * per;
    return {p0, p0 + per < HW ? p0 + per : HW};
}

// the keep rule of SSDN_OP_HEAD_VJP: a sample whose request is exactly the forward's d mean(LOSS) (keep, no g_pme / g_mu, w[b] == 1.f/B)
// leaves its g_net_out and partials alone.  (Scalars, not the argument struct by reference: taking the kernel argument's address in a
// kernel that otherwise does not changes how the compiler contracts the arithmetic downstream.)
static __device__ __forceinline__ bool head_vjp_kept(int keep, const float* g_pme, const float* g_mu, const float* w, float wb, int B) {
    return keep && !g_pme && !g_mu && w && wb == 1.f / (float)B;
}

struct Sym3 { float m00, m01, m02, m11, m12, m22; };
// Sigma_x = U U^T, U = [[a0,a1,a2],[0,a3,a4],[0,0,a5]]   (denoiser.py:246-255)
static __device__ __forceinline__ Sym3 sym3_uut(const float* A) {
    Sym3 x;
    x.m00 = A[0] * A[0] + A[1] * A[1] + A[2] * A[2];
    x.m01 = A[1] * A[3] + A[2] * A[4];
    x.m02 = A[2] * A[5];
    x.m11 = A[3] * A[3] + A[4] * A[4];
    x.m12 = A[4] * A[5];
    x.m22 = A[5] * A[5];
    return x;
}
// s + diag(d0, d1, d2)
static __device__ __forceinline__ Sym3 sym3_add_diag(const Sym3& s, float d0, float d1, float d2) {
    return {s.m00 + d0, s.m01, s.m02, s.m11 + d1, s.m12, s.m22 + d2};
}
static __device__ __forceinline__ Sym3 sym3_scale(const Sym3& s, float k) {
    return {s.m00 * k, s.m01 * k, s.m02 * k, s.m11 * k, s.m12 * k, s.m22 * k};
}
// adjugate of a symmetric 3x3 matrix; returns its determinant
static __device__ __forceinline__ float sym3_adj(const Sym3& s, Sym3& c) {
    c.m00 = s.m11 * s.m22 - s.m12 * s.m12; c.m01 = s.m02 * s.m12 - s.m01 * s.m22; c.m02 = s.m01 * s.m12 - s.m02 * s.m11;
    c.m11 = s.m00 * s.m22 - s.m02 * s.m02; c.m12 = s.m01 * s.m02 - s.m00 * s.m12; c.m22 = s.m00 * s.m11 - s.m01 * s.m01;
    return s.m00 * c.m00 + s.m01 * c.m01 + s.m02 * c.m02;
}
// o = (m v) k
static __device__ __forceinline__ void sym3_mv(const Sym3& m, const float* v, float k, float* o) {
    o[0] = (m.m00 * v[0] + m.m01 * v[1] + m.m02 * v[2]) * k;
    o[1] = (m.m01 * v[0] + m.m11 * v[1] + m.m12 * v[2]) * k;
    o[2] = (m.m02 * v[0] + m.m12 * v[1] + m.m22 * v[2]) * k;
}
// dL/dU = 2 G U on the upper triangle, G = dL/dSigma_x as a symmetric matrix (dL/dx01 as a scalar = 2 G01)
static __device__ __forceinline__ void sym3_dldu(const Sym3& G, const float* A, float* g) {
    g[0] = 2.f * (G.m00 * A[0]);
    g[1] = 2.f * (G.m00 * A[1] + G.m01 * A[3]);
    g[2] = 2.f * (G.m00 * A[2] + G.m01 * A[4] + G.m02 * A[5]);
    g[3] = 2.f * (G.m01 * A[1] + G.m11 * A[3]);
    g[4] = 2.f * (G.m01 * A[2] + G.m11 * A[4] + G.m12 * A[5]);
    g[5] = 2.f * (G.m02 * A[2] + G.m12 * A[4] + G.m22 * A[5]);
}
