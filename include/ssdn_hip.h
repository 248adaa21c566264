/*
 * ssdn_hip.h -- C-ABI of libssdn_hip.so: the MI355X (gfx950 / CDNA4) hot path of the `ssdn`
 * blind-spot denoising trainer.
 *
 * The reference (COMP6248-Reproducability-Challenge/selfsupervised-denoising) is pure PyTorch and has
 * NO FFI for this path: every "kernel" below replaces an ATen/cuDNN op the
 * reference launches implicitly through torch.nn.  Each entry point cites the reference code it
 * replaces.  The boundary carries plain pointers and sizes only -- no torch types.  The host side
 * (Python, like the reference) keeps the reference's module API (NoiseNetwork / Denoiser) and lowers
 * one forward / training step to a flat list of `ssdn_op` records executed by ssdn_run_ops().
 *
 * Conventions
 *   - all device pointers are caller-owned (the Python host allocates them with torch on the
 *     current device); the library allocates nothing and keeps no state besides the last error.
 *   - activation tensors: NHWC, 16-bit, `cs` = elements per pixel (channel stride), `co` = channel offset
 *     of this view inside the pixel, so concatenations / channel slices are views, never copies.
 *     FORWARD activations are fp16 (11-bit significand: the eval PSNR budget of +-0.05 dB needs it);
 *     every GRADIENT tensor of the backward pass is bf16 (fp32 exponent range: the SSDN loss gradient spans > 7 decades
 *     between pixels when sigma is estimated / Poisson, which no fp16 loss scale can hold) -- accumulation is fp32 always.
 *   - every function returns 0 on success; on failure a negative code and ssdn_last_error() gives text.
 *     No C++ exception crosses the boundary.
 *   - `stream` is a hipStream_t (NULL = the default stream); all work is enqueued asynchronously.
 *   - not thread-safe per stream; one host thread per GPU (one process per GPU).
 */
#ifndef SSDN_HIP_H
#define SSDN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: the functions declared here are its whole dynamic symbol table */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define SSDN_ABI_VERSION 19
#define SSDN_MAX_TAPS 9

/* NHWC fp16 view: element (n,y,x,c) lives at p[((n*H + y)*W + x)*cs + co + c]. */
typedef struct ssdn_view {
    void* p;
    int32_t cs;
    int32_t co;
} ssdn_view;

enum ssdn_op_type {
    SSDN_OP_PACK_INPUT = 1, /* rotate-stack + NCHW f32 -> NHWC f16 */
    SSDN_OP_CONV = 2,       /* implicit-GEMM MFMA convolution (forward or data-gradient role) */
    SSDN_OP_POOL_FWD = 3,
    SSDN_OP_POOL_BWD = 4,
    SSDN_OP_UPSUM_BWD = 5,
    SSDN_OP_UNROT_FWD = 6,
    SSDN_OP_UNROT_BWD = 7,
    SSDN_OP_WGRAD = 8,
    SSDN_OP_WREDUCE = 9,
    SSDN_OP_WPACK = 10,
    SSDN_OP_GRAD_PACK = 11,
    SSDN_OP_HEAD_SSDN = 12,
    SSDN_OP_HEAD_FINAL = 13,
    SSDN_OP_SPATIAL_MEAN = 14,
    SSDN_OP_MSE = 15,
    SSDN_OP_MASK_MSE = 16,
    SSDN_OP_ADAM = 17,
    SSDN_OP_METRICS = 18,  /* per-step loss / PSNR / std-dev sums into a device-resident accumulator (H11) */
    SSDN_OP_ZERO = 19,
    SSDN_OP_EVENT_RECORD = 20, /* hipEventRecord(event) on the op's lane: lets a consumer outside the list (the gradient
                                  all-reduce on its own stream) wait for a PREFIX of the list */
    SSDN_OP_NOISE = 21,        /* training patch stream: uint8 clean patches -> noisy / clean / reference fp32 (+ Noise2Void) */
    SSDN_OP_INPUT_GRAD = 22,   /* gradient w.r.t. the network input (NoiseNetwork under autograd with x.requires_grad) */
    SSDN_OP_HEAD_VJP = 23,     /* vector-Jacobian product of the SSDN head: any upstream gradient of LOSS / posterior mean / mu */
    SSDN_OP_MSE_VJP = 24,      /* the same for the (masked) MSE pipelines: LOSS / network output */
    SSDN_OP_ACCUM = 25,        /* dst[i] = fl(dst[i] + src[i]): folds a per-pass staging value into a running gradient sum */
    SSDN_OP_HEAD_POSTERIOR = 26, /* per-pixel posterior of the SSDN head beyond its mean: covariance, std maps, samples (no planned list holds it) */
    SSDN_OP_SSIM = 27,          /* per-sample SSIM of two image batches over each sample's un-padded extent, optional SSIM map (no planned list holds it) */
    SSDN_OP_CALIBRATION = 28,   /* per-sample calibration statistics of the posterior N(mean, cov) against the clean image, optional z histogram / z map (no planned list holds it) */
    SSDN_OP_IMAGE_IN = 29,      /* whole uint8 images of differing sizes -> the padded fp32 input batch: / 255, transposed, reflection-padded (no planned list holds it) */
    SSDN_OP_IMAGE_OUT = 30,     /* an fp32 batch -> uint8 images of differing sizes: cropped to each extent, clipped, * 255, truncated, transposed (no planned list holds it) */
    SSDN_OP_NOISE_EST = 31,     /* a blind per-image noise-level estimate (gauss sigma, poisson lambda) from the packed uint8 images SSDN_OP_IMAGE_IN reads (no planned list holds it) */
    SSDN_OP_TILE_IN = 32,       /* one uint8 image of any size -> a batch of its fixed-size overlapping tiles: / 255, transposed, reflected beyond the image (no planned list holds it) */
    SSDN_OP_TILE_OUT = 33,      /* the fp32 tiles of one image -> that image, blended across the overlaps: bytes or upright fp32 planes (no planned list holds it) */
    SSDN_OP_POOL_PATCH = 34,    /* a minibatch of training patches cut out of a device-resident pool of uint8 images: crop, dihedral transform, / 255 (+ Noise2Void) (no planned list holds it) */
    SSDN_OP_IMAGE_IN16 = 35,    /* SSDN_OP_IMAGE_IN for packed uint16 images: min(s, white) / white (no planned list holds it) */
    SSDN_OP_IMAGE_OUT16 = 36,   /* SSDN_OP_IMAGE_OUT writing uint16: clipped, * white, rounded to nearest even (no planned list holds it) */
    SSDN_OP_TILE_IN16 = 37,     /* SSDN_OP_TILE_IN from one uint16 image (no planned list holds it) */
    SSDN_OP_TILE_OUT16 = 38,    /* SSDN_OP_TILE_OUT's blend, quantised to uint16 [h][w][C] (no planned list holds it) */
    SSDN_OP_POOL_PATCH16 = 39,  /* SSDN_OP_POOL_PATCH over a planar uint16 pool (no planned list holds it) */
    SSDN_OP_RISK = 40           /* per-sample reference-free risk statistics of the SSDN head's two outputs from the noisy image alone (no planned list holds it) */
};

/* One record of the op list.  `args` points at the matching ssdn_*_args struct (host memory).
 * lane 0: the op is enqueued on the caller's stream.  Lanes 1..3 are library-owned side streams:
 *   lanes 1 and 3 run an op AFTER everything that precedes it in the list on lane 0 (and on their own lane);
 *   lane 2 runs an op AFTER everything that precedes it in the list on lanes 0, 1 and 3 (and on lane 2).
 * The executor inserts the hipEvent dependencies; a lane never waits for a lane it does not depend on inside a list, but
 * ssdn_run_ops joins all side streams back into the caller's stream before it returns.  The planner guarantees the absence
 * of WAR/WAW hazards between lanes: lanes 1 and 3 carry (alternately) the weight-gradient GEMMs of the backward pass (they
 * read tensors written once per step and write their OWN slab), lane 2 the slab reductions (they read that slab and write
 * the flat gradient, which nothing else touches) -- so the many small, latency-bound backward launches overlap instead of
 * queueing behind each other.  (The planner's guarantee is checked, channel range by channel range, by
 * tests/test_lane_hazards_cpu.py against the model in tests/lane_model.py; the executor's ordering by tests/test_hip_lanes.py.) */
typedef struct ssdn_op {
    int32_t type;
    int32_t lane;
    const void* args;
} ssdn_op;

/* ---- SSDN_OP_PACK_INPUT ----------------------------------------------------------------------
 * replaces: the 4-rotation batch stacking, noise_network.py:187-189 + utils/data.py:42-67 (flip/transpose/cat),
 * and the NCHW-f32 -> NHWC-f16 layout change.  dst[r*B+b, i, j, c] = rot_r(src[b,c])[i,j], r=0..R-1,
 * rot = (0,90,180,270) with rotate(x,90)[i,j] = x[j, W-1-i]; channels c >= C are written as zero. */
typedef struct ssdn_pack_input_args {
    const float* src; /* [B,C,H,W] f32 */
    ssdn_view dst;    /* [R*B,H,W,cs] f16 */
    int32_t B, C, H, W;
    int32_t R;        /* 4 (blind-spot) or 1 */
    int32_t cpad;     /* channels written (>= C, zero padded) */
} ssdn_pack_input_args;

/* ---- SSDN_OP_CONV ------------------------------------------------------------------------------
 * replaces: ShiftConv2d / nn.Conv2d (+bias) + LeakyReLU(0.1) + nn.Upsample(nearest) + torch.cat
 * (noise_network.py:58,70-156,200-210,241-260) in the forward role, and autograd's conv data-gradient in the
 * backward role.  Computes, for every output pixel (n,y,x) and m < M:
 *     v = bias[m] + sum_{t<ntaps} sum_{k<Ktot} Wp[t][m][k] * IN(n, y+dy[t], x+dx[t], k)
 *     if act:  v = v > 0 ? v : 0.1 v
 *     if add:  v += add(n,y,x,m)
 *     if mask: v *= (mask(n,y,x,m) > 0 ? 1 : 0.1)             (LeakyReLU' of a saved activation)
 * IN is the virtual channel-concatenation [src0 (c0 ch), src1 (c1 ch)], zero outside [0,H)x[0,W);
 * src0 is read at (y>>1, x>>1) when up0 (nearest 2x upsample folded into the load).
 * Wp is fp16 [ntaps][Mpad][Ktot] (packed by SSDN_OP_WPACK), Ktot = c0+c1 (multiple of 16), Mpad multiple of 32.
 * Output: dst (16-bit NHWC view) or, when dst32 != NULL, fp32 NCHW planar [N][M][H][W] (net_out).
 * bf16 = 0: src0/src1/w/dst/add are fp16 (forward role).  bf16 = 1: they are bf16 (data-gradient role); `mask` is
 * always an fp16 saved activation. */
typedef struct ssdn_conv_args {
    ssdn_view src0;
    ssdn_view src1;
    int32_t c0, c1, up0;
    int32_t N, H, W;
    int32_t ntaps;
    int32_t dy[SSDN_MAX_TAPS];
    int32_t dx[SSDN_MAX_TAPS];
    const void* w; /* fp16 [ntaps][Mpad][Ktot] */
    int32_t M, Mpad, Ktot;
    const float* bias; /* [M] or NULL */
    int32_t act;
    ssdn_view mask; /* p == NULL: none */
    ssdn_view add;  /* p == NULL: none */
    ssdn_view dst;
    float* dst32;
    /* tiling chosen by the host (see ssdn/hip/graph.py): tile = 2^ltn images x 2^lth rows x 2^ltw cols = 256 px */
    int32_t ltw, lth, ltn;
    int32_t kc; /* channel chunk staged in LDS at a time (multiple of 16, divides Ktot) */
    int32_t bf16;
    const void* wc; /* optional second copy of the weights for the persistent LDS-DMA kernel (k_cdma), or NULL: chunk-major and
                       pre-swizzled, [tap][chunk][Mpad][kc] with kc = 48 (chunks of 48 input channels, then one optional 16-channel
                       chunk); the 16-byte piece p of row m is stored at piece p ^ ((m >> 3) & 1) -- exactly the LDS image, so a
                       (tap, chunk) slice is one linear, fully coalesced DMA (SSDN_OP_WPACK writes it: wfc / wdc) */
    int32_t kreal; /* real (un-padded) input channels among the Ktot slots (0: = Ktot): the algorithmic flop count of the profiler, and a
                      CONTRACT for the forward role -- the input channels >= kreal are zero (SSDN_OP_PACK_INPUT pads with zeros), so a
                      launch may skip them (k_conv_thin, csrc/conv_thin.hip, serves Ktot = 16 with kreal <= 3) */
    /* Fused Shift2d((1,0)) + nn.MaxPool2d(2) of the conv's activated 16-bit output (SSDN_OP_POOL_FWD semantics; the reference:
     * noise_network.py:64-67): pool.p != NULL makes the epilogue ALSO write pooled[N,H/2,W/2,M] -- the max is taken over the
     * rounded fp16 values the epilogue stores, so the result is bit-identical to SSDN_OP_POOL_FWD applied to dst.  Only the
     * launches ssdn_conv_fuses_pool() accepts can do this (today: forward layers whose 256-pixel tile is made of whole images,
     * i.e. 16x16 pixels and below at BASELINE sizes); any other launch with pool.p set is an error. */
    ssdn_view pool;
    int32_t pool_shifted;
    /* Fused SSDN_OP_UPSUM_BWD (data-gradient role of a decoder's first conv, whose input is cat(upsample(x), skip)):
     * upsum.p != NULL => output channels [0, upsum_c) are NOT stored to dst; their 2x2 sums (over the bf16-rounded values, in
     * fp32, window scan order) times LeakyReLU'(upsum_mask) are stored to upsum[N,H/2,W/2,..] -- bit-identical to
     * SSDN_OP_UPSUM_BWD applied to the tensor this launch would have stored.  Channels >= upsum_c (the skip gradient) go to
     * dst as usual.  Needs bf16 = 1, no mask / add, even H, W; upsum_c a multiple of 8 -- and of 96 for the launches that
     * run k_cdma.  ssdn_conv_fuses_upsum() tells whether a launch can do it; otherwise upsum.p set is an error. */
    ssdn_view upsum;
    ssdn_view upsum_mask;
    int32_t upsum_c;
    /* Fused SSDN_OP_UNROT_BWD (data gradient of the first 1x1 head layer of a blind-spot network, whose input is the
     * un-rotated stack of the four rotated feature maps): unrot.p != NULL => nothing is stored to dst; output channel block r
     * (of M / 4 channels) of pixel (b, i, j) goes to unrot[(r * N + b), u - 1, v, :] times LeakyReLU'(unrot_mask there), with
     * (u, v) the rotated coordinates of SSDN_OP_UNROT_FWD; the pixels with u == 0 (cut off by the shift) write the zero row
     * y = H - 1 instead -- the complete tensor SSDN_OP_UNROT_BWD would have produced, bit-identical.  N of the conv = batch;
     * needs bf16 = 1, a 1x1 layer with M = 384, H == W a power of two, no mask / add (ssdn_conv_fuses_unrot()). */
    ssdn_view unrot;
    ssdn_view unrot_mask;
    /* optional: the sign bytes SSDN_OP_UNROT_FWD wrote for unrot_mask's tensor (ssdn_unrot_args.smask); when set they are read
     * instead of unrot_mask (same result: only the sign of the activation enters LeakyReLU'). */
    const void* unrot_smask;
    /* fused SSDN_OP_UNROT_FWD (forward role; replaces: rotate(x, -90k) + Shift2d((1,0)) + torch.cat of noise_network.py:213-222 applied
     * to this layer's output).  When urot.p is set the launch is the layer over the four rotated copies of a batch (N = 4B images
     * r*B + b, H == W = P, M = Mpad = 96): the output pixel (rB+b, y, x), y <= P-2, is stored at urot[b, i, j, r*M + m] -- the
     * place SSDN_OP_UNROT_FWD would have moved it to -- and nothing goes to dst (which may be null); row y = P-1 is dropped and the
     * rows of urot the one-row shift leaves empty are NOT written (they stay zero in a zero-initialised tensor).  urot_smask,
     * optional: the LeakyReLU sign bytes of the output (ssdn_unrot_args.smask).  ssdn_conv_fuses_urot() tells whether a launch can. */
    ssdn_view urot;
    void* urot_smask;
    /* LeakyReLU sign bytes instead of saved activations in the backward pass (both optional; ssdn_conv_signs() tells whether a launch
     * honours them): sign_out (forward role, 16-bit dst) -- the launch also writes one byte per 8 output channels, bit q of byte
     * [pixel][k] = (output channel 8k+q > 0), [N*H*W][M/8]; mask_sign (data-gradient role) -- such bytes for the tensor `mask` views,
     * read instead of it (same result: only the sign of the activation enters LeakyReLU'; 1/16 of the bytes); upsum_mask_sign
     * (data-gradient role with the fused SSDN_OP_UPSUM_BWD) -- such bytes for the tensor `upsum_mask` views, [N*(H/2)*(W/2)][upsum_c/8]. */
    void* sign_out;
    const void* mask_sign;
    const void* upsum_mask_sign;
} ssdn_conv_args;

/* ---- SSDN_OP_POOL_FWD / SSDN_OP_POOL_BWD ----------------------------------------------------
 * replaces: Shift2d((1,0)) + nn.MaxPool2d(2) (noise_network.py:64-67, models/utility.py:37-53) and its autograd
 * backward fused with the LeakyReLU backward of the producing conv.
 * shifted: window rows {2i-1, 2i}, row -1 is a literal 0 that takes part in the max; else rows {2i, 2i+1}.
 * BWD: dz(n,y,x,c) = (first position in window scan order whose value equals the pooled max is (y,x))
 *                    ? dpool(n,i,j,c) * (act > 0 ? 1 : 0.1) : 0;  if the zero pad row wins the gradient is dropped.
 * route (optional, uint32 [N,H/2,W/2,C/8]): FWD also writes one word per (window, 8 channels) -- nibble q of channel 8k+q: bits 0-1 = scan
 *   position of the first maximum, bit 2 = the zero pad row holds it, bit 3 = the maximum is > 0; BWD launched on its own reads the word
 *   instead of the four activation pieces of the window (same result, 4 bytes instead of 64; a chained launch keeps reading `act`). */
typedef struct ssdn_pool_args {
    ssdn_view act;    /* [N,H,W,C] full-res post-activation */
    ssdn_view pooled; /* [N,H/2,W/2,C]  (FWD: output, BWD: input) */
    ssdn_view dpool;  /* BWD only */
    ssdn_view dz;     /* BWD only: [N,H,W,C] */
    int32_t N, H, W, C;
    int32_t shifted;
    void* route;
} ssdn_pool_args;

/* ---- SSDN_OP_UPSUM_BWD ----------------------------------------------------------------------
 * replaces: autograd backward of nn.Upsample(nearest, 2x) + LeakyReLU backward of the producer.
 * dst(n,i,j,c) = (sum_{a,b<2} src(n,2i+a,2j+b,c)) * (mask(n,i,j,c) > 0 ? 1 : 0.1); dims are those of dst. */
typedef struct ssdn_upsum_args {
    ssdn_view src;  /* [N,2H,2W,..] */
    ssdn_view mask; /* [N,H,W,..] */
    ssdn_view dst;  /* [N,H,W,..] */
    int32_t N, H, W, C;
} ssdn_upsum_args;

/* ---- SSDN_OP_UNROT_FWD / SSDN_OP_UNROT_BWD --------------------------------------------------
 * replaces: final Shift2d((1,0)), chunk(4), un-rotate (0,270,180,90), cat(dim=1) (noise_network.py:213-222).
 * FWD: dst[b,i,j,r*C+c] = S_r(src)[..], S_r[y,x] = y>=1 ? src[r*B+b, y-1, x] : 0, rotated back by (0,270,180,90).
 * BWD: the adjoint, times LeakyReLU'(act) of the tensor that was un-rotated. */
typedef struct ssdn_unrot_args {
    ssdn_view src;  /* FWD: [4B,P,P,C] ; BWD: [B,P,P,4C] (gradient) */
    ssdn_view dst;  /* FWD: [B,P,P,4C] ; BWD: [4B,P,P,C] */
    ssdn_view mask; /* BWD only: [4B,P,P,C] saved activation */
    int32_t B, P, C;
    /* FWD, optional: [4B,P,P,C/8] bytes, bit q of byte k = (src channel 8k+q > 0) -- the LeakyReLU sign of every pixel the
     * un-rotation reads (rows y <= P-2; row P-1 is cut off by the shift and left untouched).  The fused backward
     * (ssdn_conv_args.unrot_smask) reads these 12 bytes per pixel instead of the 192-byte activation. */
    void* smask;
} ssdn_unrot_args;

/* ---- SSDN_OP_WGRAD --------------------------------------------------------------------------
 * replaces: autograd's conv weight/bias gradient.  dz is bf16, IN is fp16 (converted to bf16 while it is staged in
 * LDS; products are exact in the fp32 accumulator).  Every workgroup s < nslabs reduces its share of pixels into
 *   slab[s][t][m][k] = sum_pixels dz(n,y,x,m) * IN(n, y+dy[t], x+dx[t], coff[t]+k)   (fp32, [nslabs][ntaps][Mpad][Kpad])
 *   bslab[s][m]      = sum_pixels dz(n,y,x,m)
 * IN as in SSDN_OP_CONV.  Deterministic: fixed pixel->workgroup assignment, SSDN_OP_WREDUCE sums slabs in order. */
typedef struct ssdn_wgrad_args {
    ssdn_view dz; /* [N,H,W,..] gradient w.r.t. the conv's pre-activation output, M channels */
    ssdn_view src0;
    ssdn_view src1;
    int32_t c0, c1, up0;
    int32_t N, H, W;
    int32_t ntaps;
    int32_t dy[SSDN_MAX_TAPS];
    int32_t dx[SSDN_MAX_TAPS];
    int32_t coff[SSDN_MAX_TAPS]; /* channel offset of tap t inside IN: lets the "taps" of a 1x1 layer be channel blocks */
    int32_t M, Mpad, Ktot, Kpad; /* Ktot = channels staged; every tap covers channels [coff[t], coff[t]+Kpad) */
    float* slab;
    float* bslab;
    int32_t nslabs;
    int32_t ltw, lth, ltn; /* pixel tile per iteration: 2^ltn x 2^lth x 2^ltw */
    int32_t csplit;        /* column groups G (0 or 1: none).  The output is ntaps*Kpad/32 + 1 column tiles of 32 (tile 0 = the
                              bias column); with G > 1 a workgroup owns ceil(tiles / G) consecutive ones and the grid is
                              nslabs x G: for layers with few pixels, where writing a full slab per workgroup (~10 B per
                              clock per CU) and reading it back would dominate */
    int32_t mblocks;       /* >= 1: the launch covers mblocks blocks of M output channels (dz channels [b*M, b*M+M) of the dz
                              view, slabs [b*nslabs, (b+1)*nslabs) of `slab` / `bslab`): grid = mblocks x nslabs workgroups,
                              the mblocks workgroups that stream the same pixels placed on one XCD so that the input tile
                              reaches HBM once (1x1 head layers: 4 blocks of 96) */
    int32_t kreal;         /* real (un-padded) input channels among the Ktot slots, or 0 (unknown).  1..3 real channels under a
                              3x3 window (the network's first layer and the image half of decode_block_1.0) are served by the
                              im2col kernel k_wgrad_thin: 9 * kreal + 1 <= 32 GEMM columns instead of 9 x 32 */
    int32_t mega;          /* > 0: the op is planned as part of ONE merged launch (k_wgrad_mega) together with the SSDN_OP_WGRAD ops next
                              to it in the list that carry the same value (the number of CUs the planner sized the group's grids
                              for): every block of every op's grid becomes one block of the merged launch, sorted by `cost`,
                              longest first, so that the CUs pick them up in that order; each block runs the code of its op's own
                              launch (bit-identical slabs).  0: the op is launched on its own */
    float cost;            /* planner's estimate of the time of ONE block of this op's grid, any unit (only the ratios matter) */
} ssdn_wgrad_args;

/* ---- SSDN_OP_WREDUCE ------------------------------------------------------------------------
 * gw[m][cin][ky][kx] (fp32 OIHW, the checkpoint layout) = inv_scale * sum_s slab[s][t][m][k(cin)],
 * gb[m] = inv_scale * sum_s bslab[s][m];  k(cin) = cin (cin < c0) else c0 + (cin - c0) i.e. padding removed:
 * real input channels are [0,c0) and [c0, c0+c1_real).  inv_scale is read from device memory (loss-scale word).
 * Slabs are summed in a fixed order, every sum a chain of fp32 adds that starts from 0.f: bit-reproducible.  Weights: groups of 32
 * slabs in index order, then the group sums in order (nslabs <= 32: one chain over all slabs).  Bias: ONE chain over all slabs in
 * index order, no groups (bslab is never used as scratch).  The sum is multiplied by inv_scale with one rounding.
 * (tests/test_hip_optimiser.py holds the device to this order bit for bit.)
 * NOTE: the slab buffer is used as scratch (partial sums are written back into it).
 * accumulate = 1 (gradient accumulation over micro-batches): the epilogue ADDS instead of storing,
 *   gw[o] = fl(gw[o] + fl(inv_scale * sum)),  gb[m] = fl(gb[m] + fl(inv_scale * sum)):
 * the product is rounded first, then one fp32 add (no FMA), so the running sum is fl(old + g) with g bit for bit what
 * accumulate = 0 stores.  Elements that accumulate = 0 does not write (padding, gb == NULL) stay untouched either way.
 * The flag is a property of a RUN: the caller sets it on the argument structs, the planner's records do not carry it. */
typedef struct ssdn_wreduce_args {
    const float* slab;
    const float* bslab;
    int32_t nslabs, ntaps, M, Mpad, Kpad;
    int32_t cin;      /* real input channels covered by this slab (k < cin are real, the rest is padding) */
    int32_t cin_full; /* input channels of the whole weight tensor (row length of gw) */
    int32_t m_off, c_off; /* this slab is the block gw[m_off.., c_off..] (the 1x1 head layers are computed in blocks) */
    int32_t tapblock;     /* 1: the slab's "taps" are channel blocks of a 1x1 layer: input channel = c_off + t*Kpad + k */
    float* gw;
    float* gb; /* may be NULL (bias gradient is produced by one block column only) */
    const float* inv_scale; /* device scalar, may be NULL (=1) */
    int32_t accumulate;     /* 0: store (overwrite gw / gb), 1: add to what gw / gb hold */
} ssdn_wreduce_args;

/* ---- SSDN_OP_WPACK --------------------------------------------------------------------------
 * fp32 OIHW master weights -> the two fp16 shadows the MFMA kernels read:
 *   wf[t][m][k]  (forward role)  = W[m][cin(k)][t]  for m < M, k real; 0 in the padding   [ntaps][Mpad_f][Ktot]
 *   wd[t][c][m]  (dgrad role)    = W[m][cin(c)][t]   stored as bf16                       [ntaps][Mpad_d][Kd]
 * k -> cin: k < c0 ? k : (k - c0 < c1_real ? c0 + k - c0 : padding). */
typedef struct ssdn_wpack_args {
    const float* w; /* [M][cin][ntaps] */
    void* wf;
    void* wd; /* may be NULL (first layer needs no data gradient) */
    int32_t M, cin, ntaps;
    int32_t c0, c1_real;
    int32_t Mpad_f, Ktot; /* forward shadow dims */
    int32_t Mpad_d, Kd;   /* dgrad shadow dims: Mpad_d >= Ktot, Kd >= M (multiple of 16) */
    void* wfc;            /* optional chunk-major pre-swizzled copies of wf / wd (see ssdn_conv_args.wc), same sizes; NULL: none. */
    void* wdc;            /* Only for Ktot (resp. Kd) = 48 n or 48 n + 16 */
} ssdn_wpack_args;

/* ---- SSDN_OP_GRAD_PACK ----------------------------------------------------------------------
 * fp32 NCHW gradient w.r.t. net_out -> bf16 NHWC [N,H,W,cpad] (zero padded channels).  bf16 keeps the fp32 exponent
 * range, so there is NO loss scaling; scale_out[0] = scale_out[1] = 1 is written for SSDN_OP_WREDUCE's inv_scale input.
 * gmax (float bits of max |g|, written by the loss kernels with atomicMax) is kept as an overflow / NaN sentinel: a running maximum --
 * the host clears it (SSDN_OP_ZERO) when it wants a per-step figure. */
typedef struct ssdn_grad_pack_args {
    const float* g; /* [N,C,H,W] */
    ssdn_view dst;
    int32_t N, C, H, W, cpad;
    const uint32_t* gmax; /* float bits of max |g| */
    float* scale_out;     /* [2] */
} ssdn_grad_pack_args;

/* ---- SSDN_OP_HEAD_SSDN / SSDN_OP_HEAD_FINAL -------------------------------------------------
 * replaces: Denoiser._ssdn_pipeline (denoiser.py:218-397) and its autograd backward:
 * per-pixel Gaussian posterior algebra in closed form (3x3 SPD inverse/det by adjugate), fp32.
 *   style: 0 gauss, 1 poisson, 2 impulse.   mode: 0 known, 1 const (one learnable scalar), 2 var (sigma-net, one value / sample)
 *   noise_param[b]: sigma (gauss), lambda (poisson) or alpha (impulse) for mode known.   est_raw: [1] (const) or [B] (var), pre-softplus.
 * Outputs (any may be NULL): mu / pme [B,C,H,W], model_std [B,H,W], noise_std [B] (gauss, impulse: alpha) or [B,H,W] (poisson),
 *   g_net_out [B,Cout,H,W] = d mean(LOSS) / d net_out, partial[b][chunk][2] = {sum loss, sum dloss/dest_raw} per workgroup,
 *   gmax = atomicMax of |g| float bits.
 * HEAD_FINAL sums the partials in fixed order: loss[b] = mean over pixels; g_est (const: [1], var: [B]);
 *   for var also fills g_sigma_out [B,1,H,W] with g_est[b]/(H*W) (gradient of the spatial mean) and folds it into gmax2.
 * diag (ABI 18): 0 = the full covariance above; 1 = DIAGONAL_COVARIANCE: Cout = 2*C, net_out = [mu_c, a_c], Sigma_x = diag(a_c^2),
 *   per-channel closed forms, g_net_out [B,2*C,H,W]; with C = 1 both are the same model (bit for bit).
 *   C must be 1 or 3.
 * style 2, IMPULSE (a new VALUE of `style`, no layout change: the ABI version stays; csrc/head_impulse.hip): with
 *   probability alpha a pixel was replaced, in all channels, by a colour uniform on (0,1]^C.  alpha: known: clamp(noise_param[b], 1e-3,
 *   0.999); const / var: min(softplus(est_raw - 4) + 1e-3, 0.999), no gradient through an active clamp.  With e = mu_x - 1/2:
 *     mu_y = alpha/2 + (1 - alpha) mu_x,  Sigma_y = (1 - alpha) Sigma_x + alpha/12 I + alpha (1 - alpha) e e^T   (the mixture's moments)
 *     l = 1/2 log det Sigma_y + 1/2 (y - mu_y)^T Sigma_y^-1 (y - mu_y)   (C = 1: log sy + d^2 / sy);  l -= 0.1 alpha for mode != known
 *     pme = mu_x + w (y - mu_x),  w = sigmoid(log(1 - alpha) - log alpha + log N(y; mu_x, Sigma_x + 1e-6 I))
 *   mu = mu_x, model_std as style 0, noise_std[b] = alpha.  diag = 1 with style 2 is an error. */
typedef struct ssdn_head_args {
    const float* net_out; /* [B,Cout,H,W] */
    const float* noisy;   /* [B,C,H,W] */
    const float* noise_param;
    const float* est_raw;
    int32_t B, C, H, W;
    int32_t style, mode;
    int32_t want_grad;
    float* mu;
    float* pme;
    float* model_std;
    float* noise_std;
    float* g_net_out;
    float* partial;
    int32_t nchunks;
    uint32_t* gmax;
    int32_t diag;         /* ABI 18: 1 = diagonal covariance (see above), 0 = full */
} ssdn_head_args;

typedef struct ssdn_head_final_args {
    const float* partial;
    int32_t B, nchunks, H, W;
    int32_t mode;
    float* loss;        /* [B] */
    float* g_est;       /* [1] or [B] */
    float* g_sigma_out; /* var: [B,1,H,W] */
    uint32_t* gmax2;    /* var: max |g_sigma_out| bits */
} ssdn_head_final_args;

/* mean over H,W of a [B,1,H,W] fp32 map (denoiser.py:264) */
typedef struct ssdn_spatial_mean_args {
    const float* src;
    float* dst;
    int32_t B, HW;
} ssdn_spatial_mean_args;

/* ---- SSDN_OP_MSE / SSDN_OP_MASK_MSE ---------------------------------------------------------
 * replaces: Denoiser._mse_pipeline (denoiser.py:153-154) / loss_mask_mse (utils/n2v_loss.py:6-17, quirk kept:
 * coordinates of batch element 0 are used for every element, squared errors summed over coordinates, mean over C).
 * loss[b]; g = d mean_b(loss) / d out (fp32 NCHW); gmax as above. */
typedef struct ssdn_mse_args {
    const float* out; /* [B,C,H,W] */
    const float* ref;
    const int64_t* coords; /* MASK_MSE: [ncoords][2] (row, col) of batch element 0 */
    int32_t ncoords;
    int32_t B, C, H, W;
    float* loss;
    float* g;
    uint32_t* gmax;
} ssdn_mse_args;

/* ---- SSDN_OP_HEAD_VJP / SSDN_OP_MSE_VJP ----------------------------------------------------------
 * replaces: autograd's backward through Denoiser._ssdn_pipeline / _mse_pipeline / _mask_mse_pipeline (denoiser.py:140-397) for ANY
 * upstream gradient of the pipeline's differentiable outputs, not just d mean(LOSS) (Denoiser.run_pipeline under autograd).
 * Upstream gradients (any may be NULL = no gradient for that output): w[b] = dL/dLOSS[b]; g_pme = dL/dIMG_DENOISED [B,C,H,W];
 * g_mu = dL/dIMG_MU [B,C,H,W] (ssdn only).  HEAD_VJP writes g_net_out = dL/dnet_out [B,Cout,H,W], the per-workgroup partials
 * partial[b][chunk][1] of dL/dest_raw (same layout / chunking as SSDN_OP_HEAD_SSDN; partial[..][0], the loss sums, are left alone),
 * then reduces them in HEAD_FINAL's order into g_est (const: [1], var: [B]) and, for var, g_sigma_out = g_est[b]/(H*W).
 * MSE_VJP writes g = w[b] dLOSS[b]/dout + g_pme (masked: the coordinates of batch element 0, duplicates counted, as SSDN_OP_MASK_MSE).
 * |g| is folded into gmax (gmax2: |g_sigma_out|).  Per-pixel math: DESIGN.md section 3.8.
 * keep = 1 declares that g_net_out / g and the partials still hold what the forward's loss op wrote (d mean(LOSS)): then a sample
 * with no g_pme / g_mu and w[b] == 1.f/B exactly keeps them untouched (the check runs on the device), so mean(LOSS) under autograd
 * is bit-identical to the planned backward pass at every batch size.  Every reduction is in a fixed order: bit-reproducible.
 * g_noisy (ABI 17; NULL = not computed, every other output unchanged bit for bit): HEAD_VJP also writes the head's DIRECT term of
 * dL/dnoisy [B,C,H,W] -- net_out and sigma held fixed; a sample that keeps g_net_out (keep) still writes it.
 * diag (ABI 18): the forward's diag (SSDN_OP_HEAD_SSDN): 1 = the diagonal-covariance head, net_out / g_net_out [B,2*C,H,W].
 * style 2 (impulse, see SSDN_OP_HEAD_SSDN): the same contract -- w, g_pme, g_mu, keep, g_est / g_sigma_out = dL/dest_raw through alpha,
 *   g_noisy (y enters y - mu_y, log N(y; ..) and w (y - mu_x)); diag = 1 with style 2 is an error. */
typedef struct ssdn_head_vjp_args {
    const float* net_out; /* [B,Cout,H,W] */
    const float* noisy;   /* [B,C,H,W] */
    const float* noise_param;
    const float* est_raw; /* [1] (const) or [B] (var), pre-softplus */
    int32_t B, C, H, W;
    int32_t style, mode;
    const float* w;       /* [B] or NULL */
    const float* g_pme;   /* [B,C,H,W] or NULL */
    const float* g_mu;    /* [B,C,H,W] or NULL */
    int32_t keep;
    int32_t nchunks;      /* = the forward's */
    float* g_net_out;
    float* partial;       /* [B][nchunks][2] */
    uint32_t* gmax;
    float* g_est;         /* const: [1], var: [B], known: NULL */
    float* g_sigma_out;   /* var: [B,1,H,W] */
    uint32_t* gmax2;      /* var */
    float* g_noisy;       /* [B,C,H,W] or NULL (ABI 17) */
    int32_t diag;         /* ABI 18: = the forward's */
} ssdn_head_vjp_args;

typedef struct ssdn_mse_vjp_args {
    const float* out;     /* [B,C,H,W] */
    const float* ref;
    const int64_t* coords; /* masked: [ncoords][2] (row, col) of batch element 0 */
    int32_t ncoords;
    int32_t masked;
    int32_t B, C, H, W;
    int32_t keep;
    const float* w;       /* [B] or NULL */
    const float* g_pme;   /* [B,C,H,W] or NULL */
    float* g;             /* [B,C,H,W] */
    uint32_t* gmax;
} ssdn_mse_vjp_args;

/* ---- SSDN_OP_ADAM ---------------------------------------------------------------------------
 * replaces: torch.optim.Adam.step over all parameters (train.py:100-107,202): one fused pass over the flat fp32
 * master buffer.  p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps), bc = 1 - beta^step (host computes bc1, bc2). */
typedef struct ssdn_adam_args {
    float* p;
    const float* g;
    float* m;
    float* v;
    int64_t n;
    float lr, b1, b2, eps, bc1, bc2;
    float gscale; /* multiplies g first (1/world_size for data parallel) */
} ssdn_adam_args;

/* ---- SSDN_OP_METRICS ------------------------------------------------------------------------
 * H11: the per-step metric accumulation of the trainer / evaluator (reference train.py:205-218,553-584, utils/data.py:94-105 with
 * utils/utils.py Metric.add) as ONE launch that adds into a device-resident accumulator; the host reads the 16 floats back when it
 * prints (PRINT_INTERVAL), not every step.  Per sample b, over the valid extent ext[b] = (e1, e2) of the two spatial axes (NULL:
 * the whole image -- evaluation batches are padded, metadata IMAGE_SHAPE):
 *     psnr_x[b]   = -10 log10( mean_{c, i < e1, j < e2} (x[b,c,i,j] - clean[b,c,i,j])^2 )     x = out (IMG_DENOISED), mu (IMG_MU)
 *     mstd[b]     = 255 * mean_{i,j} model_std[b,i,j]          nstd[b] = 255 * noise_std[b] (or its mean over the pixels)
 * and acc[2k] += sum_b value_k[b], acc[2k+1] += count_k for k = 0..4 = loss, psnr_out, psnr_mu, noise_std, model_std (count = B; 1
 * for a noise_std that is one value for the whole batch) -- exactly what `Metric.add` of the reference accumulates (sum over the
 * samples of the per-sample value, sample count).  Deterministic: per-sample values go through `per`, the block that arrives last
 * (ticket in acc[15]) adds them in a fixed order (deterministic).  NULL inputs are skipped. */
typedef struct ssdn_metrics_args {
    const float* out;       /* [B,C,H,W] or NULL */
    const float* mu;        /* [B,C,H,W] or NULL */
    const float* clean;     /* [B,C,H,W] */
    const float* loss;      /* [B] or NULL */
    const float* model_std; /* [B,H,W] or NULL */
    const float* noise_std; /* [noise_n] values (noise_n = 1, B or B*H*W) or NULL */
    const int32_t* ext;     /* [B][2] or NULL */
    int32_t B, C, H, W;
    int32_t noise_n;
    float* per;             /* scratch [B][8] */
    float* acc;             /* [16] accumulator (the host zeroes it when it resets its metrics) */
} ssdn_metrics_args;

typedef struct ssdn_zero_args {
    void* p;
    int64_t bytes;
} ssdn_zero_args;

/* ---- SSDN_OP_ACCUM ---------------------------------------------------------------------------
 * dst[i] = fl(dst[i] + src[i]), i < n: one fp32 add per element.  An accumulating backward pass of a model with a learnable noise
 * scalar (mode const) points g_est of SSDN_OP_HEAD_FINAL / SSDN_OP_HEAD_VJP at a one-float staging buffer and folds it into the flat
 * gradient with this op, once per pass (those ops STORE g_est: writing the flat gradient directly would destroy the running sum). */
typedef struct ssdn_accum_args {
    float* dst;
    const float* src;
    int64_t n;
} ssdn_accum_args;

/* ---- SSDN_OP_EVENT_RECORD -------------------------------------------------------------------
 * Records the caller-owned hipEvent_t `event` on the stream of the op's lane, i.e. after every earlier op of that lane (and,
 * through the lane dependencies, after the lane-0 ops those depend on).  Data parallelism (replaces nn.DataParallel's
 * reduce, denoiser.py:102-110): the host puts one after the last weight-gradient reduction of each gradient bucket and lets
 * the RCCL stream wait for it, so a bucket's all-reduce overlaps the rest of the backward pass. */
typedef struct ssdn_event_args {
    void* event;
} ssdn_event_args;

/* ---- SSDN_OP_NOISE --------------------------------------------------------------------------
 * replaces the per-sample preparation of the training stream, reference ssdn/ssdn/datasets/noise_wrapper.py:66-135 with
 * utils/noise.py:54-107 (add_gaussian / add_poisson) and utils/n2v_ups.py:40-88 (Noise2Void pixel selection), for a whole
 * minibatch of CLEAN uint8 patches already on the device:
 *     clean   = u8 / 255
 *     param   = p_lo                                   if p_lo == p_hi
 *               U[p_lo, p_hi) per (sample, CHANNEL)    otherwise (the reference draws a ranged parameter per leading index of an
 *                                                      unbatched CHW sample, i.e. per channel: noise.py:34-39,55-56)
 *     gauss:    noisy = clean + param * N(0,1)                       (param = std dev as a fraction of 1)
 *     poisson:  noisy = (clean * param + Poisson(1)) / param         (RATE-1 noise on lambda x: the reference's quirk, noise.py:101-104)
 *     impulse:  noisy = Bernoulli(param) per PIXEL ? U(0,1]^C : clean   (style 2: one decision for all channels of a pixel, the untouched
 *               pixel stays exactly u8 / 255; param = alpha in [0, 1], ONE draw per sample for a range, written to all C entries of
 *               param[b*C + c]; C <= 3; clip has nothing to do; the decision and the colours are a pure function of (seed, offset,
 *               stream, pixel), so the Noise2Void copy and ref32 work as for the other styles)
 *     clip:     noisy = min(max(noisy, 0), 1)
 * `ref32` (optional) is a second, independent realisation with its own parameter draw (the Noise2Noise / Noise2Void reference).  With n2v_box > 0 the
 * first realisation is manipulated like n2v_ups.manipulate: one pixel (c0, c1) per n2v_box x n2v_box box (c0 stratified over W,
 * c1 over H, uniform inside the box), replaced in every channel by the noisy value of a pixel drawn uniformly from
 * [min(c - r, 0), min(c + r, size - 1)) without c itself, per axis (the reference's window: [0, c + r) in the interior, negative
 * indexes wrap like Python's); coords[b][i * (H / box) + j] = (c0, c1) as the reference returns them (image[:, c1, c0] is the
 * replaced pixel).  Random numbers: Philox4x32-10 keyed by `seed`, counter = (element, stream, offset): stateless, every launch
 * must pass a fresh `offset`.  The distributions are the reference's; the random STREAM is not torch's (parity of the noise with the
 * reference package is statistical by construction; the stream itself is pinned, element by element, against the
 * host model tests/philox_ref.py).  The uniform values behind every draw lie in (0, 1]: 24 bits of a word, centred, and the top one
 * rounds up to 1.0 in fp32. */
typedef struct ssdn_noise_args {
    const void* clean_u8; /* [B,C,H,W] uint8 */
    float* clean32;       /* out [B,C,H,W] or NULL */
    float* noisy32;       /* out [B,C,H,W] */
    float* ref32;         /* out [B,C,H,W] or NULL */
    float* param;         /* out [B*C] or NULL: the parameter of the first realisation */
    float* param_ref;     /* out [B*C] or NULL: the (independently drawn) parameter of the second realisation */
    int64_t* coords;      /* out [B, (W/box)*(H/box), 2] or NULL (required when n2v_box > 0) */
    int32_t B, C, H, W;
    int32_t style;        /* 0 gauss, 1 poisson, 2 impulse */
    int32_t clip;
    float p_lo, p_hi;
    int32_t n2v_box;      /* 0: no manipulation */
    int32_t n2v_radius;   /* sub-patch radius (2 for the reference's 5 x 5) */
    uint64_t seed, offset;
} ssdn_noise_args;

/* ---- SSDN_OP_HEAD_POSTERIOR --------------------------------------------------------------------
 * The per-pixel posterior N(pme, Sigma_post) the head of SSDN_OP_HEAD_SSDN implies (impulse: a two-component mixture), beyond its mean:
 * csrc/head_posterior.hip, DESIGN.md section 3.13.  net_out, noisy, noise_param, est_raw, B, C, H, W, style, mode, diag, nchunks are
 * ssdn_head_args' (the same sigma_c, alpha, est and Sigma_x = U U^T rules).  Sigma_post is the matrix M with pme = M (Sx'^-1 mu + Sn'^-1 y)
 * in the form that arm of the head evaluates (e = 1e-6):
 *   full, C = 3: K Sn' symmetrised, K = Sx' T^-1, Sx' = Sigma_x + e I, Sn' = diag(sigma_c^2) + e I, T = Sx' + Sn';  C = 1: sx sn / sy;
 *   diag = 1, C = 3: diag(1 / (1/(sx_c + e) + 1/(sn_c + e) + e));  style 2: (1 - w) Sigma_x + w (1 - w) r r^T, r = y - mu_x, w the head's.
 * Outputs (any may be NULL, not all): cov [B, C(C+1)/2, H, W], upper triangle in the order 00, 01, 02, 11, 12, 22 (C = 1: [B,1,H,W]);
 *   std [B,C,H,W] = sqrt(max(diagonal, 0));  samples [n_samples, B, C, H, W]: pme + L z with L L^T = Sigma_post (Cholesky, pivots clamped
 *   at 0); style 2: y exactly with probability w, else mu_x + U z.  Random numbers: Philox4x32-10 keyed by `seed`, counter = (b H W + pixel,
 *   0x80000000 + 2 s + k, offset): sample s is a pure function of (seed, offset, s, b, pixel) -- independent of n_samples and nchunks --
 *   and shares no stream with SSDN_OP_NOISE.  B H W < 2^32.  Adding this op changed no existing struct: the ABI version stays.
 * Argument errors are raised before any device call (text prefixed "head_posterior:"); diag = 1 with style 2 is an error. */
typedef struct ssdn_head_posterior_args {
    const float* net_out; /* [B,Cout,H,W] */
    const float* noisy;   /* [B,C,H,W] */
    const float* noise_param;
    const float* est_raw;
    int32_t B, C, H, W;
    int32_t style, mode;
    int32_t diag;
    int32_t nchunks;
    float* cov;
    float* std;
    float* samples;
    int32_t n_samples;    /* >= 1 when samples is given */
    uint64_t seed, offset;
} ssdn_head_posterior_args;

/* ---- SSDN_OP_SSIM ------------------------------------------------------------------------------
 * The structural similarity index of Wang, Bovik, Sheikh and Simoncelli (2004) with the parameters of the authors' code: the window
 * g[k] ~ exp(-(k - 5)^2 / (2 * 1.5^2)), k = 0..10, normalised to sum 1, applied separably as an 11 x 11 window at the positions where the
 * whole window lies inside the image (no padding: an h x w image has (h - 10) x (w - 10) positions).  Per channel and position, E[.] the
 * window-weighted sum:  mx = E[x], my = E[ref], sxx = E[x^2] - mx^2, syy = E[ref^2] - my^2, sxy = E[x ref] - mx my,
 *     SSIM = (2 mx my + C1)(2 sxy + C2) / ((mx^2 + my^2 + C1)(sxx + syy + C2)),   C1 = 0.01^2, C2 = 0.03^2 (data range 1; nothing is clipped)
 * ssim[b] = the plain mean over the channels and the positions of sample b's image, which is its un-padded extent ext[b] = (e1, e2) of
 * the two spatial axes (SSDN_OP_METRICS' convention; NULL: the whole image).  ext is device memory: the kernel clamps it to [0,H] x [0,W].
 * A sample whose extent is below 11 in either axis has no position: ssim[b] = NaN and nothing of its map is written.
 * map (optional): the value of the window over rows i..i+10, columns j..j+10 goes to its centre, map[b,c,i+5,j+5]; every other element
 * is left untouched.
 * Arithmetic (csrc/ssim.hip): fp32 in; the five window sums, the formula and the mean in fp64 (the products of
 * fp32 values are exact there, so E[x^2] - mx^2 does not cancel in the working precision); one rounding to fp32 per stored value.  One
 * workgroup per (SSDN_SSIM_TILE_H x SSDN_SSIM_TILE_W tile of positions, channel, sample), tiles counted from (0,0) of the extent; each
 * adds its positions in a fixed order into scratch, and a second launch adds a sample's tile sums in a fixed order that depends on the
 * extent alone: ssim[b] does not depend on the padding around the extent, on map being requested or on the launch being repeated.
 * scratch: device memory of SSDN_SSIM_SCRATCH_BYTES(B, C, H, W) bytes, 8-byte aligned, contents irrelevant before and after.
 * Argument errors are raised before any device call (text prefixed "ssim:"): x, ref, ssim or scratch NULL, B or C < 1, H or W < 11,
 * scratch_bytes below the rule, B * C or the tile rows above 65535.  Adding this op changed no existing struct: the ABI version stays. */
#define SSDN_SSIM_WIN 11
#define SSDN_SSIM_TILE_H 16
#define SSDN_SSIM_TILE_W 32
#define SSDN_SSIM_TILES(n, t) (((n) - (SSDN_SSIM_WIN - 1) + (t) - 1) / (t))
#define SSDN_SSIM_SCRATCH_BYTES(B, C, H, W) \
    ((int64_t)8 * (B) * (C) * SSDN_SSIM_TILES(H, SSDN_SSIM_TILE_H) * SSDN_SSIM_TILES(W, SSDN_SSIM_TILE_W))
typedef struct ssdn_ssim_args {
    const float* x;       /* [B,C,H,W] */
    const float* ref;     /* [B,C,H,W] */
    const int32_t* ext;   /* [B][2] or NULL */
    int32_t B, C, H, W;
    float* ssim;          /* out [B] */
    float* map;           /* out [B,C,H,W] or NULL */
    void* scratch;        /* per-tile partial sums (fp64) */
    int64_t scratch_bytes;
} ssdn_ssim_args;

/* ---- SSDN_OP_CALIBRATION -----------------------------------------------------------------------
 * How well the per-pixel posterior N(mean, S) (SSDN_OP_HEAD_POSTERIOR's cov, upper triangle 00, 01, 02, 11, 12, 22; C = 1: the variance)
 * describes the errors actually made against the clean image ref, per sample over its un-padded extent ext[b] = (e1, e2) (SSDN_OP_METRICS'
 * convention; NULL: the whole image; device memory, clamped to [0,H] x [0,W] by the kernel).  ssdn.utils.calculate_calibration is the
 * float64 specification.  Per pixel, everything in fp64 from the fp32 inputs, r = ref - mean, in this fixed order (C = 3):
 *     p0 = s00, l00 = sqrt(p0), l10 = s01 / l00, l20 = s02 / l00;   p1 = s11 - l10^2, l11 = sqrt(p1), l21 = (s12 - l20 l10) / l11;
 *     p2 = s22 - l20^2 - l21^2, l22 = sqrt(p2);   w0 = r0 / l00, w1 = (r1 - l10 w0) / l11, w2 = (r2 - l20 w0 - l21 w1) / l22;
 *     d2 = w0^2 + w1^2 + w2^2, logdet = ln p0 + ln p1 + ln p2      (C = 1: p0 = s, d2 = r^2 / s, logdet = ln s);   z_c = r_c / sqrt(s_cc).
 * A pixel is valid iff all of its inputs are finite, every pivot p_k > 0 and every s_cc > 0; otherwise it is degenerate: counted in
 * stats[1] and left out of everything else.  stats[b][12], fp64:
 *     0: N, the valid pixels   1: the degenerate pixels   2: sum d2   3: sum logdet   4: sum |r|^2 (over channels)   5: sum tr S
 *     6, 7, 8: the (valid pixel, channel) pairs with |z_c| <= 1, 2, 3
 *     9, 10, 11: the valid pixels with d2 <= the chi^2_C quantile at 0.5, 0.9, 0.99 (SSDN_CALIB_CHI2_C1 / _C3)
 * hist (optional) [B][C][SSDN_CALIB_HIST_BINS]: counts of z_c over the valid pixels; bin 0: z < -4, bin 1 + floor(4 z + 16): -4 <= z < 4
 * (32 bins of width 0.25), bin 33: z >= 4.  zmap (optional) [B,C,H,W]: z_c, rounded once to fp32, inside the extent only (NaN at its
 * degenerate pixels); every other element is left untouched.  stats and hist of a sample with an empty extent are zeros; the op zeroes
 * what it accumulates into.
 * Arithmetic (csrc/calibration.hip): one pixel per thread, the pixels of a sample's extent numbered row-major
 * n = i * e2 + j, SSDN_CALIB_BLOCK of them per workgroup; fp64 with contraction off, so every per-pixel value is the specification's.
 * The four floating-point sums are added per workgroup in a fixed order into scratch and per sample by a second launch in an order that
 * depends on the extent alone; the counts are integers (LDS, then scratch; the histogram through atomicAdd).  Sample b's outputs do not
 * depend on the padding around its extent, on hist or zmap being requested, on the other samples or on the launch being repeated.
 * scratch: device memory of SSDN_CALIB_SCRATCH_BYTES(B, C, H, W) bytes, 8-byte aligned, contents irrelevant before and after.
 * Argument errors are raised before any device call (text prefixed "calibration:"): mean, cov, ref, stats or scratch NULL, C not 1 or 3,
 * B, H or W < 1, scratch_bytes below the rule or scratch misaligned, B above 65535 or H * W above 2^31 - 1 - SSDN_CALIB_BLOCK.
 * Adding this op changed no existing struct: the ABI version stays. */
#define SSDN_CALIB_BLOCK 256
#define SSDN_CALIB_NSTATS 12
#define SSDN_CALIB_HIST_BINS 34
#define SSDN_CALIB_CHI2_C1 { 0.45493642311957, 2.70554345409541, 6.63489660102120 }
#define SSDN_CALIB_CHI2_C3 { 2.36597388437534, 6.25138863117032, 11.3448667301444 }
#define SSDN_CALIB_SCRATCH_BYTES(B, C, H, W) \
    ((int64_t)8 * SSDN_CALIB_NSTATS * (B) * (((int64_t)(H) * (W) + SSDN_CALIB_BLOCK - 1) / SSDN_CALIB_BLOCK))
typedef struct ssdn_calibration_args {
    const float* mean;    /* [B,C,H,W] */
    const float* cov;     /* [B, C(C+1)/2, H, W] */
    const float* ref;     /* [B,C,H,W] */
    const int32_t* ext;   /* [B][2] or NULL */
    int32_t B, C, H, W;
    double* stats;                /* out [B][12] */
    unsigned long long* hist;     /* out [B][C][34] or NULL */
    float* zmap;                  /* out [B,C,H,W] or NULL */
    void* scratch;                /* per-workgroup partial sums and counts (8 bytes each) */
    int64_t scratch_bytes;
} ssdn_calibration_args;

/* ---- SSDN_OP_RISK ------------------------------------------------------------------------------
 * Judge a model without the clean image.  The blind-spot prior (mu_x, Sigma_x) at a pixel is a function of the OTHER pixels only, and for
 * the gauss and poisson heads the delivered posterior mean is affine in the pixel's own noisy value: out = mu_x + W (y - mu_x),
 * W = Sigma_x (Sigma_x + Sigma_n)^-1, W independent of y.  For zero-mean noise, independent across pixels and channels, of variance v_c:
 *     E|mu_x - x|^2 = E[ |mu_x - y|^2 - sum_c v_c ]          E|out - x|^2 = E[ |out - y|^2 + sum_c (2 W_cc - 1) v_c ]
 * (poisson: v_c = x_c / lambda has the unbiased stand-in y_c / lambda, W being independent of y_c).  The op adds the right-hand sides, the
 * Gaussian negative log-likelihood terms of y under N(mu_x, Sigma_x + Sigma_n) and what a standard error needs, per sample over the
 * margin-shrunk un-padded extent.  ssdn.utils.calculate_risk is the float64 specification; ssdn.utils.risk_values derives the reported
 * values (PSNR estimates, standard errors, NLL).
 * net_out, noisy, noise_param, est_raw, B, C, H, W, style, mode, diag are ssdn_head_posterior_args' and mean the same; style 2 (impulse:
 * neither affine nor zero-mean) is an argument error.  pme [B,C,H,W]: the output actually delivered.  The kernel builds the
 * specification's inputs itself, per pixel, widening the fp32 values to fp64 first:
 *     mu = the first C planes of net_out;  Sigma_x = U U^T (sym3_uut's sums, left to right) or diag(a_c^2) with diag = 1 (C = 1: a^2);
 *     n_c = sig^2 with head_sigma's rule: style 0: sig = (double)fmaxf(noise_param[b], 1e-3f) (mode 0) or (double)est, est head_est's fp32
 *     softplus'd estimate;  style 1: n_c = (double)fmaxf(mu_c, 1e-3f) * f, f = 1 / (double)noise_param[b] (mode 0) or (double)est;
 *     v^_c = n_c (style 0) or (double)y_c * f (style 1: the noisy value, unclipped, possibly negative).
 * Then, T = Sigma_x + diag(n_c), d = y - mu, in this fixed order (C = 3; SSDN_OP_CALIBRATION's spelling for its S):
 *     p0 = t00, l00 = sqrt(p0), l10 = t01 / l00, l20 = t02 / l00;   p1 = t11 - l10^2, l11 = sqrt(p1), l21 = (t12 - l20 l10) / l11;
 *     p2 = t22 - l20^2 - l21^2, l22 = sqrt(p2);   w0 = d0 / l00, w1 = (d1 - l10 w0) / l11, w2 = (d2 - l20 w0 - l21 w1) / l22;
 *     d2 = w0^2 + w1^2 + w2^2, logdet = ln p0 + ln p1 + ln p2;
 *     Li00 = 1 / l00, Li11 = 1 / l11, Li22 = 1 / l22, Li10 = -(l10 Li00) / l11, Li21 = -(l21 Li11) / l22, Li20 = -(l20 Li00 + l21 Li10) / l22;
 *     ti00 = Li00^2 + Li10^2 + Li20^2, ti11 = Li11^2 + Li21^2, ti22 = Li22^2 (the diagonal of T^-1);   W_cc = 1 - n_c ti_cc
 *     (C = 1: p0 = s + n, W = 1 - n / p0, d2 = d^2 / p0, logdet = ln p0);
 *     q_mu = sum_c (mu_c - y_c)^2 - sum_c v^_c,   q_out = sum_c (pme_c - y_c)^2 + sum_c (2 W_cc - 1) v^_c     (sums over c left to right).
 * There is no 1e-6 regulariser here: the heads place theirs differently (none for C = 1), far below the estimator's resolution.
 * A pixel is valid iff all of its inputs are finite and every pivot p_k > 0; otherwise it is degenerate: counted in stats[1] and left out
 * of everything else.  Only the pixels margin <= i < e1 - margin, margin <= j < e2 - margin of ext[b] = (e1, e2) take part
 * (SSDN_OP_METRICS' convention; NULL: the whole image; device memory, clamped to [0,H] x [0,W] by the kernel).  stats[b][12], fp64:
 *     0: N, the valid pixels   1: the degenerate pixels   2: sum d2   3: sum logdet   4: sum |mu - y|^2   5: sum |pme - y|^2
 *     6: sum sum_c v^_c   7: sum sum_c (2 W_cc - 1) v^_c   8: sum q_mu^2   9: sum q_out^2   10: sum tr W
 *     11: the (valid pixel, channel) pairs with y_c <= 0 or y_c >= 1: clipped samples, where the noise is not zero-mean (reported, not removed)
 * An empty region gives zeros.
 * Arithmetic (csrc/risk.hip): one pixel per thread, the pixels of the margin-shrunk region numbered row-major,
 * SSDN_RISK_BLOCK per workgroup (a function of ext and margin alone); fp64 with contraction off.  The eight floating-point sums go through
 * a fixed shuffle tree per wave, then in wave order into the workgroup's scratch slot, the three counts as integers; a second launch adds
 * a sample's slots in a fixed order.  stats[b] does not depend on the padding around the extent, on the other samples or on the launch
 * being repeated.  scratch: device memory of SSDN_RISK_SCRATCH_BYTES(B, C, H, W) bytes, 8-byte aligned, contents irrelevant before and
 * after; stats needs no initial contents either.
 * Argument errors are raised before any device call (text prefixed "risk:"): net_out, noisy, pme, stats or scratch NULL, C not 1 or 3,
 * B, H or W < 1, margin < 0, style not 0 or 1, mode not 0..2, mode 0 without noise_param or modes 1 / 2 without est_raw, diag not 0 or 1,
 * scratch_bytes below the rule or scratch misaligned, B above 65535 or H * W above 2^31 - 1 - SSDN_RISK_BLOCK.
 * Adding this op changed no existing struct: the ABI version stays. */
#define SSDN_RISK_BLOCK 256
#define SSDN_RISK_NSTATS 12
#define SSDN_RISK_SCRATCH_BYTES(B, C, H, W) \
    ((int64_t)8 * SSDN_RISK_NSTATS * (B) * (((int64_t)(H) * (W) + SSDN_RISK_BLOCK - 1) / SSDN_RISK_BLOCK))
typedef struct ssdn_risk_args {
    const float* net_out;     /* [B,Cout,H,W] */
    const float* noisy;       /* [B,C,H,W] */
    const float* noise_param; /* [B] (mode 0) */
    const float* est_raw;     /* [1] (mode 1) or [B] (mode 2) */
    const float* pme;         /* [B,C,H,W]: the output delivered */
    const int32_t* ext;       /* [B][2] or NULL */
    int32_t B, C, H, W;
    int32_t style, mode;
    int32_t diag;
    int32_t margin;
    double* stats;            /* out [B][12] */
    void* scratch;            /* per-workgroup partial sums and counts (8 bytes each) */
    int64_t scratch_bytes;
} ssdn_risk_args;

/* ---- SSDN_OP_IMAGE_IN / SSDN_OP_IMAGE_OUT ---------------------------------------------------------
 * Whole images of differing sizes into and out of the engine as bytes: what NoisyDataset.pad_to_output_size / unpad and
 * ssdn.utils.tensor2image do on the host for one image at a time, as one launch per batch and direction.
 * Images are what PIL hands out: upright uint8, row-major, channels interleaved, img[y][x][c] of h x w x C with the tight pitch w C,
 * C = 1 or 3.  The B images of a batch lie in one byte buffer, image b from byte offs[b] on; gaps between them are allowed.
 * Tensors keep the package's swapped axes (datasets/folder.py, hdf5.py): tensor axis 2 runs along the image's x, axis 3 along its y, and
 * ext[b] = (e1, e2) = (w_b, h_b) is the un-padded extent on axes 2 and 3 (SSDN_OP_METRICS' convention).  Both ops fold the transposition.
 * IMAGE_IN, every element of dst [B,C,H,W]:
 *     dst[b,c,i,j] = (float)src_b[(r(j, e2) e1 + r(i, e1)) C + c] / 255.f        (a true division, as SSDN_OP_NOISE's and to_tensor's)
 *     r(k, 1) = 0;  otherwise p = 2 (n - 1), m = k mod p, r(k, n) = m < n ? m : p - m   (numpy's "reflect" for any pad length)
 *   bit for bit to_tensor, .permute(0, 2, 1), NoisyDataset.pad_to_output_size of every image.
 * IMAGE_OUT, for x < e1, y < e2:
 *     dst_b[(y e1 + x) C + c] = q(x[b,c,x,y]),   q(v) = (uint8) trunc(fl(min(max(v, 0), 1) * 255.f)),   q(NaN) = 0
 *   which is tensor2image's np.uint8(np.clip(a, 0, 1) * 255) of the un-padded image; no byte outside an image's h_b w_b C bytes is written.
 * ext and offs are device memory the host has not seen: both kernels clamp ext to [0,H] x [0,W] and touch byte offs[b] + index only if it
 * lies inside [0, src_bytes) (dst_bytes); a read outside yields 0, a write outside is dropped, a sample with an empty extent becomes
 * zeros (in) or writes nothing (out).  Inconsistent tables never become an access outside the buffers.
 * Kernels (csrc/image_io.hip): one workgroup per (32 x 64 tile of tensor axes 2 x 3, sample) -- of the padded
 * tensor (in) or of the extent (out) --, the transposition through an LDS tile of odd pitch; bytes are touched along x, planes along axis 3.
 * Argument errors are raised before any device call (text prefixed "image_in:" / "image_out:"): a NULL pointer, C not 1 or 3, B, H or
 * W < 1, a negative byte count, B or the tile rows ceil(H / 32) above 65535.  Adding these ops changed no existing struct: the ABI version
 * stays. */
typedef struct ssdn_image_in_args {
    const uint8_t* src;   /* packed images, device */
    int64_t src_bytes;
    const int64_t* offs;  /* device [B] */
    const int32_t* ext;   /* device [B][2] = (w_b, h_b) */
    int32_t B, C, H, W;
    float* dst;           /* out [B,C,H,W]: every element is written */
} ssdn_image_in_args;

typedef struct ssdn_image_out_args {
    const float* x;       /* [B,C,H,W] */
    const int32_t* ext;   /* device [B][2] = (w_b, h_b) */
    const int64_t* offs;  /* device [B] */
    uint8_t* dst;         /* packed images out, device */
    int64_t dst_bytes;
    int32_t B, C, H, W;
} ssdn_image_out_args;

/* ---- SSDN_OP_NOISE_EST ---------------------------------------------------------------------------
 * A blind noise-level estimate per image, from the packed bytes SSDN_OP_IMAGE_IN reads (src, src_bytes, offs, ext, B, C, H, W as there:
 * image b is upright uint8 img[y][x][c] of h_b x w_b x C from byte offs[b], ext[b] = (w_b, h_b) clamped to [0,H] x [0,W]).  Nothing in
 * the reference: every path there adds the noise itself and knows its parameter.  ssdn.utils.estimate_noise is this text in float64.
 * Per 3x3 window, i.e. per (y, x, c) with 1 <= y <= h-2, 1 <= x <= w-2 (the channels pool into one table), in integers:
 *     r = sum K[dy][dx] p,  K = [[1,-2,1],[-2,4,-2],[1,-2,1]]  (Immerkaer: Var r = 36 v for i.i.d. noise of variance v; planes cancel)
 *     S = sum p;  the window is valid iff all nine bytes lie in [1, 254];  class g = (S / 9) >> 5;  bin k = min(|r|, 1023)
 * Table: hist[b][g][k] uint32 = the count of valid windows, ssum[b][g] uint64 = the sum of S over them; n_g = sum_k hist[g][k], n = sum n_g.
 * Grouped median of a histogram q of total N: half = N/2, k* the smallest k with cum(k) >= half, below = cum(k*-1), lo = max(k*-0.5, 0),
 * hi = k*+0.5, med = lo + (hi-lo)(half-below)/q[k*]; NaN if k* = 1023 (the clamp bin) or N = 0.
 * Estimates (fp64, every product, quotient and sum rounded on its own), c = 6 * 0.6744897501960817, NMIN = 256:
 *     sigma   = max(med(sum_g hist[g]) / c, 0.5) in byte units; NaN if n < NMIN
 *     per class with n_g >= NMIN: sigma_g = med(hist[g]) / c, m_g = ssum[g] / (9 n_g); the other classes are NaN and left out
 *     lambda  = min(255 sum n_g m_g^2 / sum n_g m_g sigma_g^2, 260100) over the classes kept, g ascending; a zero denominator gives the
 *               cap; NaN if no class is kept (the head's model Var = mu / lambda, in byte units 255 m / lambda)
 * est[b] = (sigma, lambda, n, classes kept, sigma_g[8], m_g[8]).  param (may be NULL): param[b] = (float)(sigma / 255) for kind 0 (gauss),
 * (float)lambda for kind 1 (poisson) -- the head's units; NaN stays NaN.
 * The op zeroes hist and ssum on its stream, counts (k_noise_est: one workgroup of 1024 threads per 64 x 32 tile of window centres and
 * sample, the tile and its one-pixel halo staged in LDS, an LDS table, integer atomics for its non-zero entries) and reduces
 * (k_noise_est_final: one workgroup per sample): integer adds commute, so the outputs are the same bits from launch to launch.  ext and offs are device memory:
 * a byte is read only inside [0, src_bytes), a byte outside counts as 0 and so invalidates its windows; wrong tables give a wrong
 * estimate, never an access outside the buffers.  Argument errors are raised before any device call (text prefixed "noise_est:"): a NULL
 * src, offs, ext, hist, ssum or est, C not 1 or 3, B, H or W < 1, a negative byte count, kind not 0 or 1, hist not 16-byte aligned,
 * B or the tile rows ceil(W / 32) above 65535.  Adding this op changed no existing struct: the ABI version stays. */
#define SSDN_NOISE_EST_CLASSES 8
#define SSDN_NOISE_EST_BINS 1024
#define SSDN_NOISE_EST_NEST 20
typedef struct ssdn_noise_est_args {
    const uint8_t* src;   /* packed images, device */
    int64_t src_bytes;
    const int64_t* offs;  /* device [B] */
    const int32_t* ext;   /* device [B][2] = (w_b, h_b) */
    int32_t B, C, H, W;
    int32_t kind;         /* 0 gauss, 1 poisson: what param receives */
    uint32_t* hist;       /* out [B][8][1024] */
    uint64_t* ssum;       /* out [B][8] */
    double* est;          /* out [B][20] */
    float* param;         /* out [B], may be NULL */
} ssdn_noise_est_args;

/* ---- SSDN_OP_TILE_IN / SSDN_OP_TILE_OUT -----------------------------------------------------------
 * One image of any size through a network of ONE fixed input shape: the image is cut into overlapping T x T tiles, every tile runs through
 * the same plan, and the tiles' outputs are blended back into one image without seams.  Nothing in the reference: it pads whole images.
 * The image is what SSDN_OP_IMAGE_IN reads: upright uint8 img[y][x][c] of h x w x C, tight pitch w C, C = 1 or 3, on the device.  Tiles keep
 * the package's swapped axes: tensor axis 2 runs along the image's x, axis 3 along its y.  tests/tile_ref.py is this text in numpy.
 * The tiling.  T: the tile edge, a positive multiple of 32 (NoiseNetwork.input_wh_mul()).  O: the overlap, a multiple of 32 with
 * 0 <= 2 O <= T.  S = T - O.  Per image axis of length n:
 *     K(n) = 1 if n <= T, otherwise ceil((n - O) / S);   origins o_k = k S, k < K(n)
 *   Every tile is T x T whatever the image (square: a blind-spot model takes it; one plan shape for a folder of pictures).  Every origin is a
 *   multiple of 32, so a tile's pooling grid is the whole image's.  The last tile may reach past n: there it sees the reflection r(., n) of
 *   SSDN_OP_IMAGE_IN (any pad length, r(k, 1) = 0).  S >= T / 2: a position is covered by one or two tiles per axis, never three, and two
 *   neighbouring tiles overlap by exactly O.  Tiles are numbered k = ky Kx + kx, row-major over the upright image, x fastest;
 *   Kx = K(w), Ky = K(h).
 *   The tiles covering position p of an axis:  kb = min(p / S, K - 1), d = p - kb S.
 *     kb >= 1 and d < O: blended -- a = tile kb - 1 at local d + S, b = tile kb at local d, t = fl32((float)(2 d + 1) / (float)(2 O))
 *     otherwise:         single  -- tile kb at local d
 *   Blend, in fp32, every operation rounded on its own (__fsub_rn, __fmul_rn, __fadd_rn, a true division: no contraction reaches it):
 *     lerp(a, b, t) = a + t (b - a), a the lower-numbered tile; first along x for each of the one or two y-tiles, then along y.
 *   lerp(a, a, t) = a for finite a, and a position under one tile is that tile's value bit for bit: tiles that agree blend to what they
 *   agree on.  NaN propagates; q(NaN) = 0 as in SSDN_OP_IMAGE_OUT.
 * TILE_IN: the tiles k0 .. k0 + B - 1 of the grid into dst [B,C,T,T], (ox, oy) the origin of tile k0 + b; every element is written:
 *     dst[b,c,i,j] = (float)src[(r(oy + j, h) w + r(ox + i, w)) C + c] / 255.f          (for a single tile: SSDN_OP_IMAGE_IN's value)
 * TILE_OUT: store is fp32 [Kx Ky, C, T, T], the network's output for every tile of the image; for every x < w, y < h:
 *     mode 0: bytes,  dst[(y w + x) C + c] = q(blend)   with SSDN_OP_IMAGE_OUT's q      (the denoised picture)
 *     mode 1: fp32,   dst[(c h + y) w + x] = blend      upright [C,h,w]                 (the posterior std map: no transposition on the host)
 *   Gather form: each output element is written once by one thread, no atomics, the same bits on every launch; nothing outside the
 *   w h C elements of dst is written.
 * Kernels (csrc/tile_io.hip): k_tile_in, one workgroup per (32 x 64 patch of tensor axes 2 x 3 of a tile, tile);
 * k_tile_out, one workgroup per (32 x 64 patch of the image's x x y): store reads run along tensor axis 3, image accesses along x, the
 * transposition goes through an LDS tile of odd pitch; offsets are 64-bit; the grid of tiles is arithmetic, there are no device tables.
 * Argument errors are raised before any device call (text prefixed "tile_in:" / "tile_out:"): a NULL pointer, C not 1 or 3, w or h < 1 or
 * above 2^30, T not a positive multiple of 32, O negative, not a multiple of 32 or 2 O > T, Kx or Ky differing from K(w), K(h),
 * w h C >= 2^31, B < 1 or a tile range outside the grid, src_bytes (dst_bytes) below what the image needs, a mode other than 0 or 1, grid
 * limits (B or T / 32 above 65535; ceil(w / 32) above 65535).  Adding these ops changed no existing struct: the ABI version stays. */
typedef struct ssdn_tile_in_args {
    const uint8_t* src;   /* the image, device */
    int64_t src_bytes;    /* >= w h C */
    int32_t w, h, C;
    int32_t T, O, Kx, Ky;
    int32_t k0, B;        /* the tiles k0 .. k0 + B - 1 */
    float* dst;           /* out [B,C,T,T]: every element is written */
} ssdn_tile_in_args;

typedef struct ssdn_tile_out_args {
    const float* store;   /* [Kx Ky, C, T, T] */
    int32_t w, h, C;
    int32_t T, O, Kx, Ky;
    int32_t mode;         /* 0: uint8 [h][w][C]; 1: fp32 [C][h][w] */
    void* dst;            /* out, device */
    int64_t dst_bytes;    /* >= w h C (mode 0), 4 w h C (mode 1) */
} ssdn_tile_out_args;

/* ---- SSDN_OP_POOL_PATCH -------------------------------------------------------------------------
 * Training on images that are ALREADY noisy: every training image is decoded once, its bytes stay on the device, and one launch cuts a whole
 * minibatch of P x P patches out of that pool.  Nothing is synthesised: the op is a gather.  tests/patch_pool_ref.py is this text in numpy.
 * The pool.  N images back to back, no alignment padding; image i is planar uint8 [C, rows_i, cols_i] at byte offsets[i], sizes[i] =
 *   (rows_i, cols_i) -- the layout of the dataset's own tensor, whatever it calls H and W.  params[i] (may be NULL): its noise parameter.
 * Sample b takes image i = index[b] (chosen on the host: the sampling order and its checkpoints stay what they are; the host checks
 *   0 <= index[b] < N before upload) and ONE Philox4x32-10 block (csrc/philox.h), counter (b, 5, offset lo, offset hi), key (seed lo,
 *   seed hi) -- stream 5 (NS_CROP) is this op's -> words v0 .. v3.  All integer arithmetic:
 *     span_x = max(cols - P, 0) + 1,  x0 = umulhi(v0, span_x);   span_y = max(rows - P, 0) + 1,  y0 = umulhi(v1, span_y)
 *     d = augment ? v2 >> 29 : 0                                 (one of the eight transforms of the square)
 * Output element (px, py) (px along tensor axis 3, py along axis 2): (u, v) = (px, py); bit 0 of d swaps u and v; bit 1: u = P - 1 - u;
 *   bit 2: v = P - 1 - v; the source is column r(x0 + u, cols), row r(y0 + v, rows) with numpy's "reflect" iterated to any length:
 *     r(t, 1) = 0;  otherwise m = t mod (2 n - 2), r(t, n) = m < n ? m : 2 n - 2 - m
 *   An image smaller than the patch is extended to the right and downwards only (the host RandomCrop pads both sides: crop positions are
 *   "distribution only" in this project).  value = (float)byte / 255.f, a true division as SSDN_OP_NOISE's.
 * Noise2Void (n2v_box > 0): the selection of one pixel per n2v_box x n2v_box box and its neighbour (rx, ry) are SSDN_OP_NOISE's, drawn from
 *   ITS coordinate stream (3) under the same (seed, offset), in patch coordinates; noisy32 at the selected pixel takes the patch value at
 *   (rx, ry) in every channel, coords[b, cell] = (c0, c1) as SSDN_OP_NOISE writes them, and ref32 is the unmanipulated patch.
 * param_out[b C + c] = params[index[b]] for every c (needs params); origin_out[b] = (x0, y0, d).
 * Kernel (csrc/patch_pool.hip): one thread per output pixel, all channels; byte addresses are 64-bit:
 *   offsets[i] + (c rows + row) cols + col.  No atomics, no LDS, no state between launches; every element of every given output is written.
 * Argument errors are raised before any device call (text prefixed "pool_patch:"): a NULL pool, offsets, sizes, index or noisy32; N, B, C or
 *   P below 1; B C P P >= 2^31; param_out without params; with n2v_box > 0: no coords, P not a multiple of n2v_box, n2v_radius < 1 or P < 2.
 * Adding this op changed no existing struct: the ABI version stays. */
typedef struct ssdn_pool_patch_args {
    const uint8_t* pool;      /* the packed images, device */
    const int64_t* offsets;   /* [N] byte offset of every image */
    const int32_t* sizes;     /* [N][2] (rows, cols) */
    const float* params;      /* [N] per-image noise parameter, may be NULL */
    const int32_t* index;     /* [B] the image of every sample */
    float* noisy32;           /* out [B,C,P,P] */
    float* ref32;             /* out [B,C,P,P], may be NULL: the unmanipulated patch */
    int64_t* coords;          /* out [B, (P / n2v_box)^2, 2], n2v_box > 0 only */
    float* param_out;         /* out [B C], may be NULL */
    int32_t* origin_out;      /* out [B][3] (x0, y0, d), may be NULL */
    int32_t N, B, C, P;
    int32_t augment;          /* 0: d = 0 */
    int32_t n2v_box, n2v_radius;
    uint64_t seed, offset;
} ssdn_pool_patch_args;

/* ---- SSDN_OP_IMAGE_IN16 / IMAGE_OUT16 / TILE_IN16 / TILE_OUT16 / POOL_PATCH16 -------------------------
 * The five byte ops above for 16-bit images: microscopy, astronomy, radiography, raw sensor data -- 12, 14 or 16 significant bits in a
 * 16-bit container.  The samples cross the bus as integers, 2 bytes each; they become the engine's fp32 on the device and come back
 * quantised.  tests/image16_ref.py is this text in numpy.  One sample model for all five:
 *   sample: a uint16 in host byte order.  white: int32 in [1, 65535], the sample value that means 1.0 (65535 full range, 4095 a 12-bit
 *     camera file: scaled by 65535 such an image would be nearly black and a noise parameter in units of white / 255 would mean nothing).
 *   in:   value = (float)min(s, white) / (float)white      one true fp32 division, as the byte ops' / 255.f; samples above white are 1.0
 *   out:  q16(v) = (uint16) rint(fl(min(max(v, 0), 1) * (float)white))      one fp32 product rounded on its own, then round to nearest,
 *     ties to even; q16(NaN) = 0, q16(-0.0) = 0.
 *   q16 rounds where SSDN_OP_IMAGE_OUT's q truncates: q follows the reference's tensor2image, q16 has no reference to follow, and
 *   truncation does not survive the round trip (white = 1000: 5 of 1001 samples come back one too low).  With rounding q16(in(s)) = s for
 *   every s <= white and every white: |fl(fl(s / white) white) - s| <= ~2 * 2^-24 * 65535 < 0.5.
 *   With white = 255 and samples that are widened bytes the "in" direction is the byte ops' value bit for bit.
 * Everything else is the sibling's definition with "byte" read as "sample": src_count, dst_count, offs[b] and the pool's offsets[i] count
 * SAMPLES, so every access is 2-byte aligned by construction.  The guard of the image ops is 0 <= offs[b] < count and
 * idx < count - offs[b]; a read outside yields 0, a write outside is dropped.
 *   IMAGE_IN16:   dst[b,c,i,j] = in(src_b[(r(j, e2) e1 + r(i, e1)) C + c])
 *   IMAGE_OUT16:  dst_b[(y e1 + x) C + c] = q16(x[b,c,x,y]) for x < e1, y < e2; no sample outside an image's h_b w_b C samples is written
 *   TILE_IN16:    dst[b,c,i,j] = in(src[(r(oy + j, h) w + r(ox + i, w)) C + c])
 *   TILE_OUT16:   dst[(y w + x) C + c] = q16(blend), SSDN_OP_TILE_OUT's blend: the same t, the same order, every operation rounded on its
 *                 own.  There is no mode: the fp32 std map goes through SSDN_OP_TILE_OUT mode 1.
 *   POOL_PATCH16: image i is planar uint16 [C, rows_i, cols_i] at sample offsets[i]; value = in(sample).  The Philox draws, crop,
 *                 transform, Noise2Void selection, coords, param_out and origin_out are SSDN_OP_POOL_PATCH's: for equal (seed, offset,
 *                 sizes, index) the two ops give equal origin_out and coords.
 * Kernels: the siblings' own, in csrc/image_io.hip, tile_io.hip and patch_pool.hip -- each kernel is one template
 * over the sample model (csrc/sample_io.h), instantiated for bytes and for uint16: one workgroup per 32 x 64 patch with the transposition
 * through an LDS tile of odd pitch holding fp32 or unsigned words (image and tile ops), one thread per output pixel (pool op).
 * Argument errors are raised before any device call, the siblings' texts under the prefixes "image_in16:", "image_out16:", "tile_in16:",
 * "tile_out16:", "pool_patch16:", and "white must lie in [1, 65535]".  Adding these ops changed no existing struct: the ABI version
 * stays. */
typedef struct ssdn_image_in16_args {
    const uint16_t* src;  /* packed images, device */
    int64_t src_count;    /* samples */
    const int64_t* offs;  /* device [B], in samples */
    const int32_t* ext;   /* device [B][2] = (w_b, h_b) */
    int32_t B, C, H, W;
    int32_t white;
    float* dst;           /* out [B,C,H,W]: every element is written */
} ssdn_image_in16_args;

typedef struct ssdn_image_out16_args {
    const float* x;       /* [B,C,H,W] */
    const int32_t* ext;   /* device [B][2] = (w_b, h_b) */
    const int64_t* offs;  /* device [B], in samples */
    uint16_t* dst;        /* packed images out, device */
    int64_t dst_count;    /* samples */
    int32_t B, C, H, W;
    int32_t white;
} ssdn_image_out16_args;

typedef struct ssdn_tile_in16_args {
    const uint16_t* src;  /* the image, device */
    int64_t src_count;    /* samples, >= w h C */
    int32_t w, h, C;
    int32_t T, O, Kx, Ky;
    int32_t k0, B;        /* the tiles k0 .. k0 + B - 1 */
    int32_t white;
    float* dst;           /* out [B,C,T,T]: every element is written */
} ssdn_tile_in16_args;

typedef struct ssdn_tile_out16_args {
    const float* store;   /* [Kx Ky, C, T, T] */
    int32_t w, h, C;
    int32_t T, O, Kx, Ky;
    int32_t white;
    uint16_t* dst;        /* out uint16 [h][w][C], device */
    int64_t dst_count;    /* samples, >= w h C */
} ssdn_tile_out16_args;

typedef struct ssdn_pool_patch16_args {
    const uint16_t* pool;     /* the packed images, device */
    const int64_t* offsets;   /* [N] sample offset of every image */
    const int32_t* sizes;     /* [N][2] (rows, cols) */
    const float* params;      /* [N] per-image noise parameter, may be NULL */
    const int32_t* index;     /* [B] the image of every sample */
    float* noisy32;           /* out [B,C,P,P] */
    float* ref32;             /* out [B,C,P,P], may be NULL: the unmanipulated patch */
    int64_t* coords;          /* out [B, (P / n2v_box)^2, 2], n2v_box > 0 only */
    float* param_out;         /* out [B C], may be NULL */
    int32_t* origin_out;      /* out [B][3] (x0, y0, d), may be NULL */
    int32_t N, B, C, P;
    int32_t augment;          /* 0: d = 0 */
    int32_t n2v_box, n2v_radius;
    int32_t white;
    uint64_t seed, offset;
} ssdn_pool_patch16_args;

/* ---- SSDN_OP_INPUT_GRAD --------------------------------------------------------------------
 * replaces: the data gradient autograd propagates into the network input through the first conv (noise_network.py:69-71) and the
 * skip half of decode_block_1's first conv (torch.cat with the input, noise_network.py:203-205), then back through the 4-rotation
 * stacking (noise_network.py:187-189).  The packed input x16 (SSDN_OP_PACK_INPUT) feeds exactly these two layers, so
 *     dx[b,c,y,x] = sum_r sum_t [ sum_{k<48} g_e0 [rB+b, p_r(y,x) - tap_t, k] * We[k][c][t]
 *                               + sum_{k<96} g_d1a[rB+b, p_r(y,x) - tap_t, k] * Wd[k][96+c][t] ]
 * with p_r the rotated position of (y,x) in rotation r (SSDN_OP_PACK_INPUT's map), tap_t = (dy[t], dx[t]) the forward taps and
 * zeros outside the image.  g_e0 / g_d1a are the PRE-activation gradients of the two layers (bf16, as the backward list leaves them).
 * The weights are read from the fp32 master buffer and rounded to bf16 inside the kernel -- the operand precision of every other data
 * gradient (the wd shadows of SSDN_OP_WPACK are bf16); accumulation is fp32.  Gather form: every output element is written once by one
 * thread, in a fixed order over (r, t, k) -- bit-reproducible, no atomics, no partial buffers.
 * Requirements: 1 <= C <= 3, R in {1, 4} (4: H == W), H and W multiples of 16, nine taps spanning at most 3 x 3, 16-byte aligned views
 * (cs, co multiples of 8) with 48 / 96 channels.
 * add (ABI 17; NULL = none): out = (the sum above) + add, add taken last -- the caller's fixed order of summing several input-gradient
 * terms.  add may alias out (each element is read once, by the thread that then writes it). */
typedef struct ssdn_input_grad_args {
    ssdn_view g_e0;      /* bf16 [R*B,H,W,cs] pre-activation gradient of encode_block_1.0 (48 channels) */
    ssdn_view g_d1a;     /* bf16 [R*B,H,W,cs] pre-activation gradient of decode_block_1.0 (96 channels) */
    const float* w_e;    /* fp32 OIHW [48][C][3][3]: encode_block_1.0 */
    const float* w_d;    /* fp32 OIHW [96][96+C][3][3]: decode_block_1.0 (input channels 96.. are the network input) */
    float* out;          /* [B,C,H,W] fp32 (overwritten) */
    int32_t B, C, H, W;
    int32_t R;           /* 4 (blind-spot) or 1 */
    int32_t ntaps;       /* 9 */
    int32_t dy[SSDN_MAX_TAPS], dx[SSDN_MAX_TAPS];   /* forward taps: the conv reads in[y + dy, x + dx] */
    const float* add;    /* [B,C,H,W] fp32 or NULL (ABI 17): added last; may alias out */
} ssdn_input_grad_args;

/* Execute `n` ops in order on `stream`.  Returns 0 or a negative error (ssdn_last_error()). */
int ssdn_run_ops(const ssdn_op* ops, int n, void* stream);

/* Order two caller streams: everything enqueued on `then` AFTER this call starts after everything enqueued on `first` BEFORE it (one event
 * of the executor's ring: hipEventRecord on `first`, hipStreamWaitEvent on `then`).  How two independent op lists run concurrently and meet
 * again -- the sigma-estimation network's lists beside the main network's (replaces the sequential execution of the two nn.Modules in
 * ssdn/ssdn/denoiser.py:261-265; DenoiserEngine._fork_sigma): order(main, side); run(list, side); order(side, main). */
int ssdn_stream_order(void* first, void* then);

/* Bytes of dynamic LDS a conv op will request (host-side check of a tiling), or < 0 if the tiling is invalid. */
int ssdn_conv_lds_bytes(const ssdn_conv_args* a);
int ssdn_wgrad_lds_bytes(const ssdn_wgrad_args* a);
/* 1 if the op (mega > 0) can be an entry of the chip-wide weight-gradient launch, 0 if it needs a launch of its own */
int ssdn_wgrad_mega_ok(const ssdn_wgrad_args* a);
/* The kernel variant the library runs the op with: out9 = {thin, MT, CPW, NL, BOTH, PS, KS, RWX, RWD}; returns the id of its
 * instance inside the chip-wide launch (>= 0), -1 if there is none, < -1 on invalid arguments.  (planner / test aid) */
int ssdn_wgrad_variant(const ssdn_wgrad_args* a, int32_t* out9);
/* The work split k_cdma (csrc/conv_dma.hip) would walk SSDN_OP_CONV with these arguments in: out8 = {tiles_x, tiles_y, segs, tps, nitems,
 * grid, xcd_map, mt_blocks} -- 16x16 tiles per image; a strip (image, tile column) is cut into `segs` work items of `tps` consecutive tiles;
 * `nitems` items on `grid` persistent workgroups (nitems > grid: workgroups take further items); xcd_map 1: each XCD walks a contiguous
 * eighth of the items, 0: item = workgroup + k * grid; mt_blocks launches, one per block of up to 96 output channels.  Computed by the
 * host code the launch itself uses, for the current device's compute units (256 without a device).  Returns 1 if the launch runs k_cdma
 * under the current ssdn_conv_set_mode, 0 if another kernel serves it (out8 is then what k_cdma would have done), < 0 on invalid
 * arguments.  (planner / test aid) */
int ssdn_conv_dma_split(const ssdn_conv_args* a, int32_t* out8);
/* The k_conv launches (csrc/conv_mfma.hip) SSDN_OP_CONV with these arguments makes under the current ssdn_conv_set_mode / _set_conv16:
 * returns their number (1 or 2: the blocks of 96 output channels, then the tail of 64 or 32), 0 if the route gives the op to another
 * kernel, < 0 with a message on invalid arguments (what the launch itself would refuse).  Per launch i, out16[8 i ..] = {MT, BF, KS, threads,
 * path, nblk, tiles, m_base}: the instantiation k_conv<MT, BF, KS, threads>; its K loop (path: 0 pipelined, 1 ASYNC -- the 1x1 LDS-DMA
 * double buffer --, 2 ALLW, 3 FLAT); nblk blocks of MT x 32 output channels from channel m_base on, each over `tiles` pixel tiles.  Computed
 * by the host code the launch itself uses, for the current device's compute units (256 without a device).  (planner / test aid) */
int ssdn_conv_variant(const ssdn_conv_args* a, int32_t* out16);

/* sizeof() of the args struct for an op type (0: ssdn_op itself); lets a binding verify its struct mirrors */
int ssdn_struct_size(int op_type);
int ssdn_abi_version(void);
const char* ssdn_last_error(void);
/* number of compute units of the current device (used to size persistent grids) */
int ssdn_device_cus(void);

/* In-stream profiler used by bench.py's roofline leg: when enabled for a kernel family, every launch of that family is
 * bracketed by a hipEvent pair ON THE LAUNCH STREAM; ssdn_profile_read() synchronises, returns the summed device time,
 * the number of launches and the ALGORITHMIC flops / bytes those launches stood for (DESIGN.md gives the formulas),
 * and resets the counters.  max_launches = 0 disables.  An event pair costs ~10 us of stream time (measured: it turns
 * back-to-back kernels into kernels with gaps), so ssdn_profile_set_stride(kind, s) brackets only every s-th launch of the
 * family: launches, flops, bytes and time then refer to the SAMPLED launches (a family's launch count per step is not a
 * multiple of the stride bench.py uses, so the sample rotates over all layers). */
#define SSDN_PROF_CONV_MT3 0
#define SSDN_PROF_CONV_MT2 1
#define SSDN_PROF_CONV_MT1 2
#define SSDN_PROF_WGRAD 3
#define SSDN_PROF_GEMM 4      /* k_gdma: 1x1 layers as one-pass LDS-DMA GEMMs */
#define SSDN_PROF_CDMA_MT3 5  /* k_cdma<3,*>: the persistent LDS-DMA 3x3 kernel on 96-channel blocks (the dominant kernel) */
#define SSDN_PROF_CDMA_MT21 6 /* k_cdma<2,*>, k_cdma<1,*> */
#define SSDN_PROF_WGRAD_SIDE 7 /* a k_wgrad_mega launch planned for fewer workgroups than the device has CUs (the side-lane launch) */
#define SSDN_PROF_KINDS 8
int ssdn_profile_enable(int kind, int max_launches);
int ssdn_profile_set_stride(int kind, int stride);
int ssdn_profile_read(int kind, double* total_ms, long long* launches, double* flops, double* bytes);

/* Which kernel serves SSDN_OP_CONV: 0 = k_conv always; 1 (default) = the persistent LDS-DMA kernel k_cdma for 3x3 layers of
 * its shape class with at least one 256-pixel tile per CU; 2 = k_cdma for every layer of its shape class (test aid). */
int ssdn_conv_set_mode(int mode);
/* 1 if SSDN_OP_CONV with these arguments writes the fused max-pool output (ssdn_conv_args.pool), 0 if it cannot. */
int ssdn_conv_fuses_pool(const ssdn_conv_args* a);
/* 1 if SSDN_OP_CONV with these arguments applies the fused SSDN_OP_UPSUM_BWD (ssdn_conv_args.upsum), 0 if it cannot. */
int ssdn_conv_fuses_upsum(const ssdn_conv_args* a);
/* 1 if SSDN_OP_CONV with these arguments applies the fused SSDN_OP_UNROT_BWD (ssdn_conv_args.unrot), 0 if it cannot. */
int ssdn_conv_fuses_unrot(const ssdn_conv_args* a);
/* 1 if SSDN_OP_CONV with these arguments stores its output un-rotated (fused SSDN_OP_UNROT_FWD, ssdn_conv_args.urot), 0 if it cannot. */
int ssdn_conv_fuses_urot(const ssdn_conv_args* a);
/* 1 if SSDN_OP_CONV with these arguments writes sign_out / reads mask_sign (whichever are set), 0 if it cannot. */
int ssdn_conv_signs(const ssdn_conv_args* a);
/* 1 if SSDN_OP_CONV with these arguments runs k_conv16 (csrc/conv16.hip): a 3x3 layer of 96 output channels (144 in the data-gradient
 * role) on whole 16x16 images, 96 or 144 input channels in 48-channel chunks, at most one image per CU, 16-bit output, no fused output
 * but the up-sum -- the launches that would otherwise run k_conv's flat path; the result is bit-identical to that path's.  Host code only.
 * ssdn_conv_set_conv16(roles): bit 0 = the forward role may run k_conv16, bit 1 = the data-gradient role may; 0 leaves every launch on
 * k_conv (test and A/B aid); -1 restores the default (the data-gradient role: profiles/conv16_ab.txt). */
int ssdn_conv16_eligible(const ssdn_conv_args* a);
int ssdn_conv_set_conv16(int roles);

/* ssdn_run_ops executes a run of consecutive ops on one lane as ONE launch (k_conv_chain, csrc/conv_chain.hip: one workgroup per
 * image walks all layers with every tensor of the run resident in LDS) when the run is a "chain":
 *   - SSDN_OP_CONV ops, all forward (bf16 = 0: bias + LeakyReLU, 16-bit output, optional fused max-pool) or all data gradients
 *     (bf16 = 1: one source, optional mask / add / fused upsum), plus -- between data gradients -- SSDN_OP_POOL_BWD ops;
 *   - 3x3 layers with identical taps and N, power-of-two images of at most 64 pixels (pooled size for SSDN_OP_POOL_BWD), kc = 48
 *     with c0, c1 multiples of 48, no dst32 / unrot;
 *   - a tensor read by an op is either written by an earlier op of the run (same p and cs, a channel window of what was written, same
 *     shape) or written by no op of the run; every output is still written to HBM.
 * The result is bit-identical to one launch per op.  ssdn_chain_len returns how many ops of the prefix of ops[0..n) run as one launch
 * (0 = none, else >= 2; at most 12; host code only, usable without a GPU); ssdn_conv_set_chain(0) switches the merging off (test
 * aid; also the folding of SSDN_OP_PACK_INPUT into the first layer's launch and of the narrow fp32-output 1x1 layer into the launch of
 * the 96-channel 1x1 layer in front of it), (1) on (default). */
int ssdn_chain_len(const ssdn_op* ops, int n);
int ssdn_conv_set_chain(int on);

/* ssdn_run_ops executes a run of consecutive SSDN_OP_WGRAD ops on one lane as ONE launch (k_wgrad_multi) when every op of the
 * run is "mergeable": at most 32768 pixels (the layers at the bottom of the U), mblocks <= 1, and a tiling the merged kernel
 * carries an instance for.  The result is bit-identical to one launch per op.  Returns 1 if `a` is mergeable, else 0. */
int ssdn_wgrad_mergeable(const ssdn_wgrad_args* a);

/* ---- step-level entry points: a whole configuration through libssdn_hip.so alone ------------------------------------------------
 * replaces: one iteration of the reference's training loop (ssdn/ssdn/train.py:196-202: run_pipeline -> mean(LOSS).backward() ->
 * optimizer.step()) and Denoiser.forward (ssdn/ssdn/denoiser.py:112-126), for ONE configuration and input shape.
 * A plan blob is written by the Python planner (DenoiserEngine.export_plan(), ssdn/hip/engine.py): the op lists of a step with every
 * pointer replaced by (tensor, offset), the tensor table, and a JSON description (configuration, shapes, the parameter layout of the
 * flat fp32 buffer: per layer name / w_off / b_off / M / cin / k, checkpoint order OIHW).  The library lays the tensors out in ONE
 * caller-owned device arena; the caller fills the named input tensors and reads the named outputs:
 *     "params" "grads" "adam_m" "adam_v"      flat fp32 buffers (a fresh arena must be ZERO: ssdn_plan_arena_bytes() bytes)
 *     "m/in32"        fp32 [B,C,H,W] network input (noisy image)          "noise_param"  fp32 [B] (ssdn, sigma known: std dev / lambda)
 *     "ref"           fp32 [B,C,H,W] reference image (mse / mask_mse)     "coords"       int64 [ncoords,2] (mask_mse)
 *     "loss"          fp32 [B]      "pme" "mu" fp32 [B,C,H,W] (ssdn: posterior mean / mu)     "m/out32" fp32 net_out
 * Phases: SSDN_PLAN_REPACK (fp16 / bf16 MFMA shadows from "params": after the caller has written parameters), SSDN_PLAN_FORWARD
 * (network + loss head), SSDN_PLAN_BACKWARD (gradients into "grads"), SSDN_PLAN_OPTIMISER (fused Adam + re-pack).  Everything is
 * enqueued asynchronously on `stream` (a hipStream_t; the library's side streams are ordered after it and joined into it).
 * Not thread-safe per plan; one plan per process / GPU.  All functions return 0 or a negative status with ssdn_last_error().
 * VALIDATED (tests/test_hip_plan_c.py, a process that imports nothing of this repository): one rank's shard of BASELINE configs 2 (ssdn,
 * sigma known), 3 (+ the sigma-estimation network: the blob concatenates the two networks' lists of a phase into ONE list, where the
 * Python path runs them as separate ssdn_run_ops calls on two streams) and 4 (Noise2Void: masked MSE at the exported coordinates) -- two
 * training steps each, loss and parameters bit-identical to the Python-driven steps.  ssdn_train_step fixes gscale = 1 and Adam's
 * betas 0.9 / 0.99 (the reference's, train.py:100-107) -- use ssdn_plan_set_lr + ssdn_plan_run for anything else. */
#define SSDN_PLAN_REPACK 0
#define SSDN_PLAN_FORWARD 1
#define SSDN_PLAN_BACKWARD 2
#define SSDN_PLAN_OPTIMISER 3
#define SSDN_PLAN_PHASES 4
typedef struct ssdn_plan ssdn_plan;
int ssdn_plan_load(const void* blob, int64_t nbytes, ssdn_plan** out);
void ssdn_plan_destroy(ssdn_plan* plan);
int64_t ssdn_plan_arena_bytes(const ssdn_plan* plan);      /* device bytes the caller provides (256-byte aligned, zero-filled) */
const char* ssdn_plan_meta(const ssdn_plan* plan);         /* the blob's JSON description */
int ssdn_plan_bind(ssdn_plan* plan, void* arena);
int ssdn_plan_tensor(const ssdn_plan* plan, const char* name, void** ptr, int64_t* bytes);
int ssdn_plan_run(ssdn_plan* plan, int phase, void* stream);
int ssdn_plan_set_lr(ssdn_plan* plan, float lr, int step, float gscale);   /* Adam: learning rate, step count (1-based: bias corrections), gradient scale */
int ssdn_net_forward(ssdn_plan* plan, void* stream);                       /* = phase SSDN_PLAN_FORWARD */
int ssdn_train_step(ssdn_plan* plan, float lr, int step, void* stream);    /* forward + loss, backward, Adam(lr, step) + re-pack */

/* Tuning aid (tools/conv_bench.py): device buffer that receives 32 s_memtime stamps per workgroup of the MFMA kernels, or
 * NULL (default) for none. */
void ssdn_debug_set_trace(void* device_buffer);
void* ssdn_debug_get_trace(void);

/* Hardware probes used by the test-suite (tests/test_hip_probe.py): raw lane mapping of
 * v_mfma_f32_32x32x16_f16 and ds_read_b64_tr_b16 on this device.  out: device buffers. */
int ssdn_probe_mfma(const void* a_frag, const void* b_frag, float* d_out, void* stream);
int ssdn_probe_tr16(const void* lds_image, int image_bytes, const int32_t* lane_addr, void* out, void* stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* SSDN_HIP_H */
