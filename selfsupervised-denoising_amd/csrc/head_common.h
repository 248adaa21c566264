// head_common.h -- what the loss-head kernel files share (head.hip, head_impulse.hip): the workgroup size, the block reductions, the
// max-|gradient| sentinel and the reference's softplus remap of a learnt noise estimate.
#pragma once
#include "common.h"

#define HB 256

static __device__ __forceinline__ float block_sum(float v, float* sh) {
    // 256 threads = 4 waves of 64
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    __syncthreads();
    if (l == 0) sh[w] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}
static __device__ __forceinline__ void atomic_max_abs(uint32_t* gmax, float v) {
    // |v| as uint is monotone in |v| for finite floats; one atomic per wave
    float a = fabsf(v);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a = fmaxf(a, __shfl_down(a, o, 64));
    if ((threadIdx.x & 63) == 0 && a > 0.f) atomicMax(gmax, __float_as_uint(a));
}
// ... one atomic per BLOCK (256 threads): the atomics of a launch all hit one address and serialise (~12 ns each); with one per wave a
// launch of one pixel per thread spent more time in them than in its arithmetic
static __device__ __forceinline__ void atomic_max_abs_block(uint32_t* gmax, float v, float* sh4) {
    float a = fabsf(v);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a = fmaxf(a, __shfl_down(a, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float m = fmaxf(fmaxf(sh4[0], sh4[1]), fmaxf(sh4[2], sh4[3]));
        if (m > 0.f) atomicMax(gmax, __float_as_uint(m));
    }
}
static __device__ __forceinline__ float softplus_m4(float raw) {
    // torch.nn.Softplus(beta=1, threshold=20) applied to (raw - 4), + 1e-3   (denoiser.py:274-275)
    float x = raw - 4.f;
    return (x > 20.f ? x : log1pf(expf(x))) + 1e-3f;
}
static __device__ __forceinline__ float sigmoid_m4(float raw) {
    float x = raw - 4.f;
    return x > 20.f ? 1.f : 1.f / (1.f + expf(-x));
}
