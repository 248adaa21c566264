// ssim.hip -- SSDN_OP_SSIM: the structural similarity index (Wang et al. 2004, 11 x 11 Gaussian window of sd 1.5, valid positions only)
// of two fp32 image batches over each sample's un-padded extent, per sample and optionally per position (gfx950).  No planned list holds it.
// Definition and contract: include/ssdn_hip.h; conditioning and measurements: DESIGN.md section 3.14.
// Arithmetic: the five window sums E[x], E[y], E[x^2], E[y^2], E[xy] are accumulated in fp64 -- the products of two fp32 values are exact
// there, so the cancellation in E[x^2] - E[x]^2 costs ~1e-12 instead of the 3e-4 of the fp32 textbook form -- and the formula and the mean
// stay in fp64: every stored value is the float64 specification (ssdn.utils.calculate_ssim) rounded once, whatever the tile shape.
// k_ssim: one workgroup per (TH x TW tile of positions, channel, sample), tiles counted from (0,0) of the extent:
//   1. the (TH + 10) x (TW + 10) halo of x and ref goes to LDS (zeros outside the extent: no valid position reads them);
//   2. row pass: for every halo row and tile column the five 11-tap sums, fp64, to LDS;
//   3. column pass: 11 taps down each of the five, the formula, the map store, and the tile's sum in a fixed order into scratch.
// k_ssim_final: one workgroup per sample adds the tile sums of its extent in an order that is a function of the extent alone.
#include "common.h"
#include <cmath>

static constexpr int SW = SSDN_SSIM_WIN, TH = SSDN_SSIM_TILE_H, TW = SSDN_SSIM_TILE_W;
static constexpr int HH = TH + SW - 1, HWD = TW + SW - 1;      // halo rows, halo columns
static constexpr int SB = 256;                                 // threads of a block (k_ssim and k_ssim_final)
static_assert(TW == 32 && (TH * TW) % SB == 0, "the column pass maps a wave's lanes to 32 consecutive columns of two rows");

struct SsimWin { double g[SW]; };                              // one table, computed in double on the host (ssim_window)

static SsimWin ssim_window() {
    SsimWin w;
    double s = 0.0;
    for (int k = 0; k < SW; ++k) s += w.g[k] = std::exp(-(double)((k - SW / 2) * (k - SW / 2)) / (2.0 * 1.5 * 1.5));
    for (int k = 0; k < SW; ++k) w.g[k] /= s;
    return w;
}

// a sample's extent, clamped to the tensor (ext is device memory: nothing on the host has seen it)
static __device__ __forceinline__ void ssim_extent(const ssdn_ssim_args& a, int b, int& e1, int& e2) {
    e1 = a.ext ? min(max(a.ext[2 * b], 0), a.H) : a.H;
    e2 = a.ext ? min(max(a.ext[2 * b + 1], 0), a.W) : a.W;
}

// the sum of one value per thread over the block, in a fixed order: a shuffle tree per wave, then the waves in wave order
static __device__ __forceinline__ double ssim_block_sum(double v, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int j = 0; j < SB / 64; ++j) t += sh[j];
    return t;
}

__global__ __launch_bounds__(SB) void k_ssim(ssdn_ssim_args a, SsimWin win) {
    __shared__ float hx[HH][HWD], hy[HH][HWD];
    __shared__ double q[5][HH][TW];
    __shared__ double red[SB / 64];
    const int b = blockIdx.z / a.C, c = blockIdx.z - b * a.C;
    int e1, e2;
    ssim_extent(a, b, e1, e2);
    const int n1 = e1 - (SW - 1), n2 = e2 - (SW - 1);           // positions of the sample per axis
    const int i0 = blockIdx.y * TH, j0 = blockIdx.x * TW;
    if (i0 >= n1 || j0 >= n2) return;                           // (block-uniform: the tile lies outside the extent, or the sample has no position)
    const long long plane = ((long long)b * a.C + c) * a.H * a.W;
    const float* px = a.x + plane;
    const float* py = a.ref + plane;
    for (int t = threadIdx.x; t < HH * HWD; t += SB) {
        const int r = t / HWD, col = t - r * HWD;
        const int i = i0 + r, j = j0 + col;
        const bool in = i < e1 && j < e2;                       // (e1 <= H, e2 <= W)
        hx[r][col] = in ? px[(long long)i * a.W + j] : 0.f;
        hy[r][col] = in ? py[(long long)i * a.W + j] : 0.f;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < HH * TW; t += SB) {
        const int r = t / TW, col = t - r * TW;
        double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
        for (int k = 0; k < SW; ++k) {
            const double x = (double)hx[r][col + k], y = (double)hy[r][col + k], g = win.g[k];
            sx += g * x;
            sy += g * y;
            sxx += g * (x * x);
            syy += g * (y * y);
            sxy += g * (x * y);
        }
        q[0][r][col] = sx; q[1][r][col] = sy; q[2][r][col] = sxx; q[3][r][col] = syy; q[4][r][col] = sxy;
    }
    __syncthreads();
    constexpr double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03;
    float* pm = a.map ? a.map + plane : nullptr;
    double acc = 0.0;
#pragma unroll
    for (int u = 0; u < TH * TW / SB; ++u) {
        const int t = threadIdx.x + u * SB;
        const int r = t / TW, col = t - r * TW;
        double s[5];
#pragma unroll
        for (int m = 0; m < 5; ++m) {
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < SW; ++k) v += win.g[k] * q[m][r + k][col];
            s[m] = v;
        }
        const double mx = s[0], my = s[1];
        const double vxx = s[2] - mx * mx, vyy = s[3] - my * my, vxy = s[4] - mx * my;
        const double val = ((2.0 * mx * my + C1) * (2.0 * vxy + C2)) / ((mx * mx + my * my + C1) * (vxx + vyy + C2));
        const int i = i0 + r, j = j0 + col;
        const bool valid = i < n1 && j < n2;
        if (valid && pm) pm[(long long)(i + SW / 2) * a.W + (j + SW / 2)] = (float)val;
        acc += valid ? val : 0.0;
    }
    const double tot = ssim_block_sum(acc, red);
    if (threadIdx.x == 0)
        reinterpret_cast<double*>(a.scratch)[((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = tot;
}

// ssim[b]: the tile sums of the sample's extent, numbered n = (c * rows + tile row) * cols + tile column; thread t adds n = t, t + SB, ...
// in that order, then the block's fixed tree; divided by the count in fp64, rounded once
__global__ __launch_bounds__(SB) void k_ssim_final(ssdn_ssim_args a, int grid_rows, int grid_cols) {
    __shared__ double red[SB / 64];
    const int b = blockIdx.x;
    int e1, e2;
    ssim_extent(a, b, e1, e2);
    const int n1 = e1 - (SW - 1), n2 = e2 - (SW - 1);
    if (n1 < 1 || n2 < 1) {                                     // (block-uniform)
        if (threadIdx.x == 0) a.ssim[b] = __builtin_nanf("");
        return;
    }
    const int rows = (n1 + TH - 1) / TH, cols = (n2 + TW - 1) / TW;
    const double* part = reinterpret_cast<const double*>(a.scratch) + (long long)b * a.C * grid_rows * grid_cols;
    const int n = a.C * rows * cols;
    double acc = 0.0;
    for (int t = threadIdx.x; t < n; t += SB) {
        const int c = t / (rows * cols), rem = t - c * (rows * cols), tr = rem / cols, tc = rem - tr * cols;
        acc += part[((long long)c * grid_rows + tr) * grid_cols + tc];
    }
    const double tot = ssim_block_sum(acc, red);
    if (threadIdx.x == 0) a.ssim[b] = (float)(tot / ((double)a.C * (double)n1 * (double)n2));
}

int launch_ssim(const ssdn_ssim_args* a, hipStream_t s) {
    if (!a->x || !a->ref) return ssdn_set_error("ssim: x and ref must be given");
    if (!a->ssim) return ssdn_set_error("ssim: the output ssim must be given");
    if (!a->scratch) return ssdn_set_error("ssim: scratch must be given");
    if (a->B < 1 || a->C < 1) return ssdn_set_error("ssim: B and C must be at least 1");
    if (a->H < SW || a->W < SW) return ssdn_set_error("ssim: H and W must be at least %d (the window)", SW);
    const long long rows = SSDN_SSIM_TILES(a->H, TH), cols = SSDN_SSIM_TILES(a->W, TW);
    if ((long long)a->B * a->C > 65535 || rows > 65535) return ssdn_set_error("ssim: B * C and the tile rows must be at most 65535");
    if (a->scratch_bytes < SSDN_SSIM_SCRATCH_BYTES((long long)a->B, a->C, a->H, a->W))
        return ssdn_set_error("ssim: scratch_bytes is below SSDN_SSIM_SCRATCH_BYTES(B, C, H, W)");
    if ((uintptr_t)a->scratch & 7) return ssdn_set_error("ssim: scratch must be 8-byte aligned");
    static const SsimWin win = ssim_window();
    hipLaunchKernelGGL(k_ssim, dim3((unsigned)cols, (unsigned)rows, (unsigned)(a->B * a->C)), dim3(SB), 0, s, *a, win);
    hipLaunchKernelGGL(k_ssim_final, dim3(a->B), dim3(SB), 0, s, *a, (int)rows, (int)cols);
    return 0;
}
