// input_grad.hip -- SSDN_OP_INPUT_GRAD: the gradient w.r.t. the network input (include/ssdn_hip.h gives the formula).
//
// One workgroup owns a 16x16 tile of one image in the UN-rotated frame and all C <= 3 channels of it.  For each rotation r:
//   1. GEMM on the matrix cores: Y[q][(t,c)] = sum_k g[q][k] * W[k][c][t] for every rotated pixel q of the tile's rotated image plus its
//      tap halo (18 x 18 pixels; 11 column blocks of 32), k over the 48 + 96 channels of g_e0 | g_d1a (nine K-steps of 16), rows (t,c) =
//      the 9 C <= 27 weight rows padded to 32.  Every gradient byte the tile needs is read ONCE per rotation (one 16-byte load per lane and
//      K-step: 8 channels of one pixel), instead of once per tap.
//   2. Y goes to LDS; each thread then gathers dx16[p][c] = sum_t Y[p - tap_t][(t,c)] for its own output pixel p = p_r(y,x) and adds it to
//      its fp32 accumulators -- the rotations meet in registers (fixed order r = 0..R-1, t = 0..8): no atomics, no cross-thread reduction.
//   3. The optional addend (another input-gradient term of the caller) is added last, per element, by the thread that writes it.
// The gradient loads of rotation r+1 are issued before the gather of rotation r (register double buffering across the barrier).
#include "common.h"

#define IG_T 16                  // output tile edge
#define IG_HALO 18               // tile + tap halo (taps span <= 3 in each axis)
#define IG_PIX (IG_HALO * IG_HALO)
#define IG_NB 11                 // 32-pixel column blocks covering the halo tile
#define IG_NS (IG_NB * 32)       // LDS row length of Y (pixel slots)
#define IG_KS 9                  // K-steps of 16 channels: 48 (g_e0) + 96 (g_d1a)
#define IG_ROWS 27               // 9 taps x C <= 3

static __device__ __forceinline__ f32x16 ig_mfma(u16x8 a, u16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// B operand of one 32-pixel column block: lane (n = lane & 31, h = lane >> 5) holds channels 16 j + 8 h .. +8 of halo pixel n
static __device__ __forceinline__ void ig_load(const ssdn_input_grad_args& a, int nimg, int i0, int j0, int blk, int lane, u16x8 (&v)[IG_KS]) {
    const int s = blk * 32 + (lane & 31), h = lane >> 5;
    const int qi = i0 + s / IG_HALO, qj = j0 + s % IG_HALO;
    const bool ok = s < IG_PIX && qi >= 0 && qi < a.H && qj >= 0 && qj < a.W;
    const long long pix = ((long long)nimg * a.H + qi) * a.W + qj;
    const unsigned short* pe = (const unsigned short*)a.g_e0.p + pix * a.g_e0.cs + a.g_e0.co + 8 * h;
    const unsigned short* pd = (const unsigned short*)a.g_d1a.p + pix * a.g_d1a.cs + a.g_d1a.co + 8 * h;
#pragma unroll
    for (int j = 0; j < IG_KS; ++j) v[j] = ok ? (j < 3 ? ld_b8(pe + 16 * j) : ld_b8(pd + 16 * (j - 3))) : zero_b8();
}

// rotated tile origin / rotated local position of the un-rotated pixel (y0 + ly, x0 + lx) (SSDN_OP_PACK_INPUT: rotate(x,90)[i,j] = x[j, W-1-i])
static __device__ __forceinline__ void ig_rot(int r, int H, int W, int y0, int x0, int ly, int lx, int& i0, int& j0, int& li, int& lj) {
    switch (r) {
        case 0: i0 = y0; j0 = x0; li = ly; lj = lx; break;
        case 1: i0 = W - IG_T - x0; j0 = y0; li = IG_T - 1 - lx; lj = ly; break;
        case 2: i0 = H - IG_T - y0; j0 = W - IG_T - x0; li = IG_T - 1 - ly; lj = IG_T - 1 - lx; break;
        default: i0 = x0; j0 = H - IG_T - y0; li = lx; lj = IG_T - 1 - ly; break;
    }
}

__global__ __launch_bounds__(256, 2) void k_input_grad(ssdn_input_grad_args a) {
    __shared__ float Y[IG_ROWS * IG_NS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = a.C, H = a.H, W = a.W, B = a.B;
    const int x0 = blockIdx.x * IG_T, y0 = blockIdx.y * IG_T, b = blockIdx.z;
    const int rows = 9 * C;
    int mdy = a.dy[0], mdx = a.dx[0];
    for (int t = 1; t < 9; ++t) { mdy = max(mdy, a.dy[t]); mdx = max(mdx, a.dx[t]); }
    const int oy = -mdy, ox = -mdx;        // halo origin relative to the rotated tile: q = p - tap, so q - p >= -max(tap)

    const int ly = tid / IG_T, lx = tid % IG_T;
    float acc[3] = {0.f, 0.f, 0.f};
    u16x8 gv[3][IG_KS];                    // column blocks wave, wave + 4, wave + 8
    int i0, j0, li, lj;
    ig_rot(0, H, W, y0, x0, ly, lx, i0, j0, li, lj);
#pragma unroll
    for (int q = 0; q < 3; ++q)            // (the first rotation's operands are in flight while the weights are fetched)
        if (wave + 4 * q < IG_NB) ig_load(a, b, i0 + oy, j0 + ox, wave + 4 * q, lane, gv[q]);

    // A operand, all nine K-steps (independent of rotation and pixel): lane (m = lane & 31, h = lane >> 5) holds row m = t C + c,
    // channels 16 j + 8 h .. +8; weights rounded to bf16 here (the data-gradient operand precision)
    u16x8 wa[IG_KS];
    {
        const int m = lane & 31, h = lane >> 5;
        const int t = m / C, c = m % C;
#pragma unroll
        for (int j = 0; j < IG_KS; ++j) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int k = 16 * j + 8 * h + e;
                float w = 0.f;
                if (m < rows) w = k < 48 ? a.w_e[(k * C + c) * 9 + t] : a.w_d[((k - 48) * (96 + C) + 96 + c) * 9 + t];
                wa[j][e] = f2bf(w);
            }
        }
    }

    for (int r = 0; r < a.R; ++r) {
        if (r > 0) __syncthreads();        // the previous rotation's gather is done with Y
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int blk = wave + 4 * q;
            if (blk >= IG_NB) continue;
            f32x16 d;
#pragma unroll
            for (int v = 0; v < 16; ++v) d[v] = 0.f;
#pragma unroll
            for (int j = 0; j < IG_KS; ++j) d = ig_mfma(wa[j], gv[q][j], d);
            // D: column (pixel) = lane & 31, row = (v & 3) + 8 (v >> 2) + 4 (lane >> 5)
            const int s = blk * 32 + (lane & 31);
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int row = (v & 3) + 8 * (v >> 2) + 4 * (lane >> 5);
                if (row < rows) Y[row * IG_NS + s] = d[v];
            }
        }
        if (r + 1 < a.R) {                 // next rotation's operands in flight during this one's gather
            int ni0, nj0, nli, nlj;
            ig_rot(r + 1, H, W, y0, x0, ly, lx, ni0, nj0, nli, nlj);
#pragma unroll
            for (int q = 0; q < 3; ++q)
                if (wave + 4 * q < IG_NB) ig_load(a, (r + 1) * B + b, ni0 + oy, nj0 + ox, wave + 4 * q, lane, gv[q]);
        }
        __syncthreads();
        ig_rot(r, H, W, y0, x0, ly, lx, i0, j0, li, lj);
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int s = (li - a.dy[t] - oy) * IG_HALO + (lj - a.dx[t] - ox);
#pragma unroll
            for (int c = 0; c < 3; ++c)
                if (c < C) acc[c] += Y[(t * C + c) * IG_NS + s];
        }
    }
    // (add, optional, comes last: out = S + add.  Each element is read and then written by this one thread, so add may alias out)
#pragma unroll
    for (int c = 0; c < 3; ++c)
        if (c < C) {
            const long long off = (((long long)b * C + c) * H + y0 + ly) * W + x0 + lx;
            a.out[off] = a.add ? acc[c] + a.add[off] : acc[c];
        }
}

int launch_input_grad(const ssdn_input_grad_args* a, hipStream_t s) {
    if (a->C < 1 || a->C > 3) return ssdn_set_error("input_grad: C = %d outside 1..3", a->C);
    if (a->R != 1 && a->R != 4) return ssdn_set_error("input_grad: R = %d (1 or 4)", a->R);
    if (a->R == 4 && a->H != a->W) return ssdn_set_error("input_grad: blind-spot rotation needs square images (H %d, W %d)", a->H, a->W);
    if (a->B < 1 || a->H < IG_T || a->W < IG_T || a->H % IG_T || a->W % IG_T || a->B > 65535)
        return ssdn_set_error("input_grad: B = %d, H = %d, W = %d (H, W multiples of %d)", a->B, a->H, a->W, IG_T);
    if (a->ntaps != 9) return ssdn_set_error("input_grad: ntaps = %d (9)", a->ntaps);
    int lo_y = a->dy[0], hi_y = a->dy[0], lo_x = a->dx[0], hi_x = a->dx[0];
    for (int t = 1; t < 9; ++t) {
        lo_y = lo_y < a->dy[t] ? lo_y : a->dy[t]; hi_y = hi_y > a->dy[t] ? hi_y : a->dy[t];
        lo_x = lo_x < a->dx[t] ? lo_x : a->dx[t]; hi_x = hi_x > a->dx[t] ? hi_x : a->dx[t];
    }
    if (hi_y - lo_y > 2 || hi_x - lo_x > 2) return ssdn_set_error("input_grad: taps span more than 3 x 3");
    if (!a->g_e0.p || !a->g_d1a.p || !a->w_e || !a->w_d || !a->out) return ssdn_set_error("input_grad: null pointer");
    if (a->g_e0.cs % 8 || a->g_e0.co % 8 || a->g_e0.co + 48 > a->g_e0.cs || ((uintptr_t)a->g_e0.p & 15))
        return ssdn_set_error("input_grad: g_e0 view must be 16-byte aligned with 48 channels (cs %d, co %d)", a->g_e0.cs, a->g_e0.co);
    if (a->g_d1a.cs % 8 || a->g_d1a.co % 8 || a->g_d1a.co + 96 > a->g_d1a.cs || ((uintptr_t)a->g_d1a.p & 15))
        return ssdn_set_error("input_grad: g_d1a view must be 16-byte aligned with 96 channels (cs %d, co %d)", a->g_d1a.cs, a->g_d1a.co);
    if ((long long)a->B * a->C * a->H * a->W >= (1ll << 31)) return ssdn_set_error("input_grad: output too large");
    SSDN_LAUNCH(k_input_grad, dim3(a->W / IG_T, a->H / IG_T, a->B), dim3(256), 0, s, *a);
    return 0;
}
