// adam_pack.h -- one element of the Adam update and one weight tile of the fused Adam + re-pack pass, shared by k_adam / k_adam_pack
// (elementwise.hip) and k_tail_fused (tail_fused.hip): the kernels must round identically and write identical shadows, so there is ONE
// copy of the arithmetic and of the shadow stores.
#pragma once
#include "common.h"

#ifndef EW_BLOCK
#define EW_BLOCK 256
#endif

// position of element (tap t, row m, column k) in the chunk-major pre-swizzled copy [tap][chunk][rows][kc] (ssdn_conv_args.wc)
static __device__ __forceinline__ long long wpack_cm(int t, int m, int k, int rows, int K) {
    const int nfull = K / 48;
    const int c = k / 48 < nfull ? k / 48 : nfull;
    const int kk = k - c * 48, kcw = c < nfull ? 48 : 16;
    const int piece = (kk >> 3) ^ ((m >> 3) & 1);
    return (long long)t * rows * K + (long long)c * 48 * rows + (long long)m * kcw + piece * 8 + (kk & 7);
}

// one element of the Adam update (shared by every optimiser kernel: explicit fmaf / no re-association)
struct AdamIn { float g, m, v, p; };
static __device__ __forceinline__ AdamIn adam_load(const ssdn_adam_args& a, long long i) { return AdamIn{a.g[i], a.m[i], a.v[i], a.p[i]}; }
static __device__ __forceinline__ float adam_apply(const ssdn_adam_args& a, long long i, const AdamIn& q, float inv_bc2s, float step) {
    const float g = q.g * a.gscale;
    const float m = __fmaf_rn(a.b1, q.m, __fmul_rn(1.f - a.b1, g));
    const float v = __fmaf_rn(a.b2, q.v, __fmul_rn(__fmul_rn(1.f - a.b2, g), g));
    a.m[i] = m;
    a.v[i] = v;
    const float den = __fmaf_rn(sqrtf(v), inv_bc2s, a.eps);
    const float pn = __fsub_rn(q.p, __fdiv_rn(__fmul_rn(step, m), den));
    a.p[i] = pn;
    return pn;
}
static __device__ __forceinline__ float adam_elem(const ssdn_adam_args& a, long long i, float inv_bc2s, float step) {
    return adam_apply(a, i, adam_load(a, i), inv_bc2s, step);
}

// ---- one weight tile: AP_TM output channels x TK input channels x all taps (TK = AP_TK, or a narrower piece of such a tile) ----------
#define AP_TM 8
#define AP_TK 48
// LDS slot of element (tap tp, row mo, column kk) of a tile that is TK channels wide
template <int TK>
static __device__ __forceinline__ int ap_slot(int tp, int mo, int kk) { return (tp * AP_TM + mo) * (TK + 1) + kk; }
// where the gradient of a tile's element comes from: the flat gradient (the only source k_adam_pack has)
struct ApGradFromMemory {
    const float* g;
    __device__ __forceinline__ float operator()(long long idx, bool, int) const { return g[idx]; }
};
// phase 1: master order; the loads of up to 7 elements of a thread are in flight together (one element at a time was a chain of 14
// exposed HBM round trips per thread).  The tile starts at output channel mo0, input channel k0 of the layer `w` whose weights begin at
// element w_off of the Adam range; gsrc(idx, ok, slot) yields the gradient of element idx (ok: the element exists; slot: its LDS slot).
// The updated parameters are parked in lds (ap_slot order), zeros where the tile hangs over the layer.
template <int NT, int TK, class GSRC>
static __device__ __forceinline__ void adam_pack_update(const ssdn_adam_args& a, const ssdn_wpack_args& w, long long w_off, int mo0, int k0,
                                                        float* lds, float inv_bc2s, float step, const GSRC& gsrc) {
    const int tid = threadIdx.x;
    constexpr int TOTAL = AP_TM * TK * NT, NIT = (TOTAL + EW_BLOCK - 1) / EW_BLOCK, BATCH = NIT < 7 ? NIT : 7;
#pragma unroll
    for (int it0 = 0; it0 < NIT; it0 += BATCH) {
        AdamIn q[BATCH];
        long long idx[BATCH];
        bool ok[BATCH];
#pragma unroll
        for (int u = 0; u < BATCH; ++u) {
            const int e = tid + (it0 + u) * EW_BLOCK;
            const int mo = e / (TK * NT), r = e - mo * (TK * NT);
            const int kk = r / NT, tp = r - kk * NT;
            ok[u] = it0 + u < NIT && e < TOTAL && mo0 + mo < w.M && k0 + kk < w.cin;
            idx[u] = ok[u] ? w_off + ((long long)(mo0 + mo) * w.cin + k0 + kk) * NT + tp : w_off;
            q[u] = AdamIn{gsrc(idx[u], ok[u], ap_slot<TK>(tp, mo, kk)), a.m[idx[u]], a.v[idx[u]], a.p[idx[u]]};
        }
#pragma unroll
        for (int u = 0; u < BATCH; ++u) {
            const int e = tid + (it0 + u) * EW_BLOCK;
            if (it0 + u >= NIT || e >= TOTAL) continue;
            const int mo = e / (TK * NT), r = e - mo * (TK * NT);
            const int kk = r / NT, tp = r - kk * NT;
            lds[ap_slot<TK>(tp, mo, kk)] = ok[u] ? adam_apply(a, idx[u], q[u], inv_bc2s, step) : 0.f;
        }
    }
}
// phases 2a / 2b: the parked tile goes out in SHADOW order (the caller has synchronised the block behind phase 1)
template <int NT, int TK>
static __device__ __forceinline__ void adam_pack_store(const ssdn_wpack_args& w, int mo0, int k0, const float* lds) {
    const int tid = threadIdx.x;
    // phase 2a: forward shadows, k fastest
    for (int e = tid; e < NT * AP_TM * TK; e += EW_BLOCK) {
        const int tp = e / (AP_TM * TK), r = e - tp * (AP_TM * TK);
        const int mo = r / TK, kk = r - mo * TK;
        const int m = mo0 + mo, k = k0 + kk;
        if (m >= w.M || k >= w.cin) continue;
        const float pn = lds[ap_slot<TK>(tp, mo, kk)];
        ((h16*)w.wf)[((long long)tp * w.Mpad_f + m) * w.Ktot + k] = (h16)pn;
        if (w.wfc) ((h16*)w.wfc)[wpack_cm(tp, m, k, w.Mpad_f, w.Ktot)] = (h16)pn;
    }
    // phase 2b: data-gradient shadows (transposed), output channel fastest
    if (w.wd) {
        for (int e = tid; e < NT * TK * AP_TM; e += EW_BLOCK) {
            const int tp = e / (TK * AP_TM), r = e - tp * (TK * AP_TM);
            const int kk = r / AP_TM, mo = r - kk * AP_TM;
            const int m = mo0 + mo, k = k0 + kk;
            if (m >= w.M || k >= w.cin || k >= w.Mpad_d || m >= w.Kd) continue;   // (the shadow may cover fewer input slots: decode_block_1.0's image channels need no gradient)
            const float pn = lds[ap_slot<TK>(tp, mo, kk)];
            ((unsigned short*)w.wd)[((long long)tp * w.Mpad_d + k) * w.Kd + m] = f2bf(pn);
            if (w.wdc) ((unsigned short*)w.wdc)[wpack_cm(tp, k, m, w.Mpad_d, w.Kd)] = f2bf(pn);
        }
    }
}
