// conv16.hip -- k_conv16: the 96-channel 3x3 layers at 16x16 pixels (decode_block_3.0 / 3.2, forward and data gradient) on a
// resident half-image tile.
//
// These launches are latency chains, not MFMA work (~2 us of matrix time per CU): as 32-channel blocks on k_conv's flat path every
// image's 18x18 halo is staged by 3..5 workgroups and every 48-channel chunk is one dependent global -> register -> LDS -> barrier round
// trip.  Here:
//   workgroup = (image, 8-row half), ALL output channels: 2 N workgroups of 4 waves; wave w owns the 32 pixels of rows 2w, 2w+1 of the
//               half (one MFMA column tile) and all MT = Mpad / 32 row tiles.
//   tile      = the 10x18 halo of the half with the WHOLE K extent, fetched by LDS-DMA (buffer_load ... lds) in one burst at kernel
//               entry: one HBM round trip per launch.  Two regions, one per source tensor ([pixel][c / 8 + 1 pieces of 16 B]: odd piece
//               stride, conflict-free ds_read_b128); the pad piece, the rows / columns outside the image and the tail of the last
//               1-KiB piece are lanes whose offset lies beyond num_records -- the hardware writes zeros.  Nearest up-sampling of
//               src0 is the (y >> 1, x >> 1) of the per-lane source offset; the channel concat is the second region.
//   weights   = streamed per (chunk, tap) slice [Mpad][48] through a ring of LDS slots by LDS-DMA from the shadow the role already has
//               (the chunk-major copy ssdn_conv_args.wc where the plan made one, else ssdn_conv_args.w), up to R slices ahead; rows are
//               7 pieces apart (6 of data + 1 zero pad).  Every wave issues its share of a slice and waits for it with a counted
//               vmcnt, then ONE barrier per step; the fragments of the next step are read while this one is on the matrix cores.
//   order     = k_conv's: chunks of 48 channels ascending, taps 0..8 inside a chunk, three K-steps ascending, the same
//               v_mfma_f32_32x32x16_{f16,bf16} with A = weights and B = pixels -- the accumulators, and with the flat path's epilogue
//               arithmetic the outputs, are bit-identical to k_conv's.
// Epilogue (k_conv's flat one on 128 pixels): bias (+LeakyReLU) in registers, tile transposed through LDS as 16-bit values, then per
// 16-byte piece the skip-gradient addend and the LeakyReLU' mask, and the fused SSDN_OP_UPSUM_BWD of the channels below upsum_c.
#include "common.h"

#define C16_THREADS 256
#define C16_HW 18                 // halo columns
#define C16_HH 10                 // halo rows of an 8-row half
#define C16_NP (C16_HW * C16_HH)
#define C16_WROW 7                // 16-byte pieces per weight row in LDS (48 channels + one pad piece)

struct C16Aux {
    int padT, padL;               // halo above / left of the tile (from the taps)
    int pa, pb;                   // pieces per pixel of region A (src0) / B (src1); 0: no such region
    unsigned mg_pa, mg_pb;        // magic reciprocals
    int rega, tile_bytes;         // bytes of region A, of both regions (multiples of 1 KiB)
};

static __device__ __forceinline__ unsigned c16_fdiv(unsigned v, unsigned magic) { return magic ? __umulhi(v, magic) : v; }
static inline unsigned c16_magic(unsigned d) { return d <= 1 ? 0u : (unsigned)((0x100000000ull + d - 1) / d); }

// one LDS-DMA piece: 64 lanes x 16 bytes to lds_dst + 16 lane.  (M0 is written in the statement that reads it.)
static __device__ __forceinline__ void c16_dma(unsigned lds_dst, int voff, u32x4_t rs) {
    asm volatile("s_nop 4\n\ts_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" :: "s"(lds_dst), "v"(voff), "s"(rs) : "memory");
}
// the LDS-DMA of a slice counts on vmcnt of the issuing wave: wait until at most N younger pieces are in flight, then the barrier
// (a plain __syncthreads() knows nothing of these loads)
template <int N>
static __device__ __forceinline__ void c16_wait_barrier() {
    asm volatile("s_waitcnt vmcnt(%0)\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier" :: "n"(N) : "memory");
}

template <bool BF>
static __device__ __forceinline__ f32x16 c16_mma(half8 av, half8 bv, f32x16 c) {
    if constexpr (BF)
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av), __builtin_bit_cast(bf16x8, bv), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(av, bv, c, 0, 0, 0);
}

// ring slots and workgroups per CU of the three instances.  Forward has the chip to itself: one workgroup per CU, a deep ring.  The data
// gradients run beside the half-chip weight-gradient launch: with at most 80 KB of LDS and 256 registers two workgroups share each of
// the free CUs, and the 2 N workgroups are one round there.
#ifndef C16_RING_F
#define C16_RING_F 8
#endif
#ifndef C16_RING_B3
#define C16_RING_B3 3
#endif
#ifndef C16_RING_B5
#define C16_RING_B5 2
#endif
#ifndef C16_OCC_B3
#define C16_OCC_B3 2
#endif
#ifndef C16_OCC_B5
#define C16_OCC_B5 2
#endif
static constexpr __host__ __device__ int c16_ring(int mt, bool bf) { return !bf ? C16_RING_F : (mt == 3 ? C16_RING_B3 : C16_RING_B5); }
static constexpr __host__ __device__ int c16_occ(int mt, bool bf) { return !bf ? 1 : (mt == 3 ? C16_OCC_B3 : C16_OCC_B5); }

template <int MT>
struct C16Frag {                  // the operands of one (chunk, tap) step: three K-steps of B (pixels) and of the MT A (weight) tiles
    half8 b[3];
    half8 a[3][MT];
};

template <int MT, bool BF>
__global__ __launch_bounds__(C16_THREADS, c16_occ(MT, BF)) void k_conv16(ssdn_conv_args a, C16Aux x) {
    constexpr int R = c16_ring(MT, BF);
    static_assert(R >= 2 && R <= 10, "ring depth");
    constexpr int WROWS = MT * 32;
    constexpr int IPW = (WROWS * C16_WROW + 255) / 256;    // LDS-DMA pieces per wave per weight slice
    constexpr int SLOT = IPW * 4 * 1024;                   // bytes of a ring slot
    constexpr int WSTR = C16_WROW * 16;
    constexpr int M = MT == 3 ? 96 : 144;                  // real output channels (the launcher checks)
    constexpr int CPP = M / 8;                             // 16-byte pieces per output pixel
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, kh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // workgroups are dealt to the 8 XCDs round-robin by id: the two halves of an image (they share two halo rows) get ids 8 apart
    const int img = (int)((blockIdx.x >> 4) * 8 + (blockIdx.x & 7)), half = (int)(blockIdx.x >> 3) & 1;
    if (img >= a.N) return;                                // (the grid is rounded up to a multiple of 16)
    // the chunk-major copy of the weights where the plan has one (ssdn_conv_args.wc: a slice is contiguous, whole 128-byte lines)
    const bool cm = a.wc != nullptr;
    // L2 warm-up (as k_cdma's): all workgroups of an XCD stream the same slices in the same order at the same time; they fetch one
    // 128-byte line per thread of the whole weight tensor before anything else
    const unsigned pf = __builtin_amdgcn_raw_buffer_load_b32(
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(cm ? a.wc : a.w), 0, 9 * a.Mpad * a.Ktot * 2, SSDN_BUFFER_RSRC_FLAGS),
        (int)(((blockIdx.x >> 3) * C16_THREADS + tid) << 7), 0, 0);

    const unsigned lds0 = (unsigned)(size_t)smem;
    const int y0 = half * 8;
    const int nchunks = a.Ktot / 48;

    // ---- the tile: one burst of LDS-DMA pieces; piece i of a region belongs to wave i % 4 ------------------------------------------
    auto stage_region = [&](const ssdn_view& v, int c, int up, int P, unsigned mgP, unsigned ldsb) __attribute__((always_inline)) {
        const int hs = up ? 8 : 16;                        // the source image is hs x hs pixels
        const unsigned long long bp = (unsigned long long)((const h16*)v.p + ((long long)img * hs * hs * v.cs + v.co));
        const u32x4_t rs = {(unsigned)bp, (unsigned)(bp >> 32) & 0xffffu, (unsigned)(((hs * hs - 1) * v.cs + c) * 2), SSDN_BUFFER_RSRC_FLAGS};
        const int total = C16_NP * P, npieces = (total + 63) >> 6;
        for (int i = wave; i < npieces; i += 4) {
            const int p = i * 64 + lane;
            const int hp = (int)c16_fdiv((unsigned)p, mgP), cc = p - hp * P;
            const int hy = hp / C16_HW, hx = hp - hy * C16_HW;
            const int y = y0 - x.padT + hy, xx = hx - x.padL;
            const bool ok = p < total && cc < P - 1 && (unsigned)y < 16u && (unsigned)xx < 16u;
            const int pix = up ? ((y >> 1) * 8 + (xx >> 1)) : (y * 16 + xx);
            c16_dma(ldsb + (unsigned)i * 1024u, ok ? (pix * v.cs + cc * 8) * 2 : (int)0x80000000, rs);
        }
    };
    if (x.pa) stage_region(a.src0, a.c0, a.up0, x.pa, x.mg_pa, lds0);
    if (x.pb) stage_region(a.src1, a.c1, 0, x.pb, x.mg_pb, lds0 + (unsigned)x.rega);

    // ---- the weight stream: slice (ch, t) = rows [0, Mpad) x channels [48 ch, 48 ch + 48) of tap t ------------------------------------
    // packed shadow w: [tap][Mpad][Ktot]; chunk-major copy wc: [tap][chunk][Mpad][48] with piece p of row m at piece p ^ ((m >> 3) & 1)
    int woff[IPW];
#pragma unroll
    for (int j = 0; j < IPW; ++j) {
        const int p = (j * 4 + wave) * 64 + lane;
        const int r = p / C16_WROW, cc = p - r * C16_WROW;
        const int src = cm ? r * 96 + ((cc ^ ((r >> 3) & 1)) << 4) : (r * a.Ktot + cc * 8) * 2;
        woff[j] = (cc < C16_WROW - 1 && r < WROWS) ? src : (int)0x80000000;
    }
    const unsigned ring = lds0 + (unsigned)x.tile_bytes;
    const unsigned wrec = cm ? (unsigned)(WROWS * 96) : (unsigned)(((WROWS - 1) * a.Ktot + 48) * 2);
    auto issue_slice = [&](int ch, int t, int slot) __attribute__((always_inline)) {
        const long long el = cm ? ((long long)(t * nchunks + ch) * a.Mpad * 48) : ((long long)t * a.Mpad * a.Ktot + ch * 48);
        const unsigned long long bp = (unsigned long long)((const h16*)(cm ? a.wc : a.w) + el);
        const u32x4_t rs = {(unsigned)bp, (unsigned)(bp >> 32) & 0xffffu, wrec, SSDN_BUFFER_RSRC_FLAGS};
#pragma unroll
        for (int j = 0; j < IPW; ++j) c16_dma(ring + (unsigned)(slot * SLOT + (j * 4 + wave) * 1024), woff[j], rs);
    };
#pragma unroll
    for (int s = 0; s < R; ++s) issue_slice(s / 9, s % 9, s);          // (a launch has at least 18 slices)

    // ---- fragments: B = this lane's pixel (MFMA column l31) of the wave's two rows, k half kh; A = weight row l31 (+ 32 mt) ---------------
    const int q = wave * 32 + l31;                         // pixel of the half: row q >> 4, column q & 15
    const int hpl = ((q >> 4) + x.padT) * C16_HW + (q & 15) + x.padL;
    const int bA = hpl * x.pa * 16 + kh * 16;
    const int bB = x.rega + hpl * x.pb * 16 + kh * 16;
    const int aoff = x.tile_bytes + l31 * WSTR + kh * 16;
    auto load_frag = [&](C16Frag<MT>& f, int ch, int dyx, int slot) __attribute__((always_inline)) {
        const bool in_a = ch * 48 < a.c0;                  // (c0 is a multiple of 48: a chunk lies in one region)
        const char* bp = smem + (in_a ? bA : bB) + (in_a ? ch * 48 : ch * 48 - a.c0) * 2 + dyx * ((in_a ? x.pa : x.pb) * 16);
        const char* ap = smem + aoff + slot * SLOT;
#pragma unroll
        for (int ks = 0; ks < 3; ++ks) {
            f.b[ks] = *reinterpret_cast<const half8*>(bp + ks * 32);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) f.a[ks][mt] = *reinterpret_cast<const half8*>(ap + mt * 32 * WSTR + ks * 32);
        }
    };

    f32x16 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;

    // Software pipeline over the steps s = 9 ch + t: the fragments of step s + 1 are read from LDS while step s is on the matrix cores.
    // At the top of step s the slices s+1 .. s+R-1 are in flight (those that exist); slice s+1 has landed in this wave's view when at most
    // the pieces of the R-2 younger ones are, and in everybody's after the barrier.  Behind the barrier every wave also holds the fragments
    // of step s in registers, so slot s % R is free for slice s + R.
    C16Frag<MT> cur, nxt;
    c16_wait_barrier<(R - 1) * IPW>();
    load_frag(cur, 0, a.dy[0] * C16_HW + a.dx[0], 0);
    for (int ch = 0; ch < nchunks; ++ch) {
        const bool last = ch + 1 == nchunks;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int s = ch * 9 + t;
            constexpr int full = (R - 2) * IPW;
            const int tail = IPW * (R - 2 < 7 - t ? R - 2 : (7 - t > 0 ? 7 - t : 0));        // last chunk: slices s+1 .. 9 nchunks - 1 remain
            if (!last) c16_wait_barrier<full>();
            else switch (tail) {                                                              // (t is a constant of the unrolled body)
                case 0: c16_wait_barrier<0>(); break;
                case IPW: c16_wait_barrier<IPW>(); break;
                case 2 * IPW: c16_wait_barrier<2 * IPW>(); break;
                case 3 * IPW: c16_wait_barrier<3 * IPW>(); break;
                case 4 * IPW: c16_wait_barrier<4 * IPW>(); break;
                case 5 * IPW: c16_wait_barrier<5 * IPW>(); break;
                case 6 * IPW: c16_wait_barrier<6 * IPW>(); break;
                default: c16_wait_barrier<0>(); break;
            }
            const int t2 = (t + R) % 9, ch2 = ch + (t + R) / 9;
            if (ch2 < nchunks) issue_slice(ch2, t2, s % R);
            const int t1 = (t + 1) % 9;
            if (t < 8 || !last) load_frag(nxt, ch + (t + 1) / 9, a.dy[t1] * C16_HW + a.dx[t1], (s + 1) % R);
#pragma unroll
            for (int ks = 0; ks < 3; ++ks)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) acc[mt] = c16_mma<BF>(cur.a[ks][mt], cur.b[ks], acc[mt]);
            cur = nxt;
        }
    }
    c16_wait_barrier<0>();                                 // tile and ring are dead: the output tile takes their place
    asm volatile("" :: "v"(pf));                           // (the warm-up load ends here)

    // ---- epilogue: k_conv's flat one.  registers -> LDS [pixel][OSTR] -> 16-byte pieces of 128 consecutive pixels --------------------
    // D row = 8 * (r >> 2) + 4 * kh + (r & 3) (output channel), D column = l31 (pixel)
    constexpr int OSTR = MT * 64 + 16;
    char* ot = smem;
    float* bl = reinterpret_cast<float*>(smem + (size_t)128 * OSTR);
    if (tid < WROWS) bl[tid] = (a.bias && tid < a.M) ? a.bias[tid] : 0.f;
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const int ml = mt * 32 + gq * 8 + kh * 4;
            const f32x4 bb = *reinterpret_cast<const f32x4*>(bl + ml);
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = acc[mt][gq * 4 + j] + bb[j];
                if (a.act) v[j] = lrelu(v[j]);
            }
            u32x2_t o;
            o[0] = BF ? pack_bf16x2(v[0], v[1]) : pack_f16x2(v[0], v[1]);
            o[1] = BF ? pack_bf16x2(v[2], v[3]) : pack_f16x2(v[2], v[3]);
            *reinterpret_cast<u32x2_t*>(ot + q * OSTR + ml * 2) = o;
        }
    }
    __syncthreads();
    const long long pixb = (long long)img * 256 + half * 128;       // first pixel of the half: its 128 pixels are consecutive in NHWC
    const bool has_mask = a.mask.p != nullptr, has_add = a.add.p != nullptr;
    constexpr int NU = 128 * CPP / C16_THREADS;                      // pieces per thread: 6 or 9, no remainder
    static_assert(128 * CPP % C16_THREADS == 0, "pieces of the half tile must divide over the threads");
    half8 mk[NU], ad[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int e = tid + u * C16_THREADS;
        const int pq = e / CPP, c = e - pq * CPP;
        mk[u] = zero_h8(); ad[u] = zero_h8();
        if (has_mask) mk[u] = ld_h8((const h16*)a.mask.p + ((pixb + pq) * a.mask.cs + a.mask.co + c * 8));
        if (has_add) ad[u] = ld_h8((const h16*)a.add.p + ((pixb + pq) * a.add.cs + a.add.co + c * 8));
    }
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int e = tid + u * C16_THREADS;
        const int pq = e / CPP, c = e - pq * CPP;
        if (a.upsum.p && c * 8 < a.upsum_c) continue;
        u32x4_t o = *reinterpret_cast<const u32x4_t*>(ot + pq * OSTR + c * 16);
        if (has_add || has_mask) {
            const u32x4_t ab = __builtin_bit_cast(u32x4_t, ad[u]), mb = __builtin_bit_cast(u32x4_t, mk[u]);
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                float v0, v1;
                if constexpr (BF) {
                    v0 = bf_lo(o[w]) + (has_add ? bf_lo(ab[w]) : 0.f);
                    v1 = bf_hi(o[w]) + (has_add ? bf_hi(ab[w]) : 0.f);
                } else {
                    v0 = f16_lo(o[w]) + (has_add ? f16_lo(ab[w]) : 0.f);
                    v1 = f16_hi(o[w]) + (has_add ? f16_hi(ab[w]) : 0.f);
                }
                if (has_mask) {
                    v0 *= lrelu_grad(f16_lo(mb[w]));
                    v1 *= lrelu_grad(f16_hi(mb[w]));
                }
                o[w] = BF ? pack_bf16x2(v0, v1) : pack_f16x2(v0, v1);
            }
        }
        *reinterpret_cast<u32x4_t*>((h16*)a.dst.p + ((pixb + pq) * a.dst.cs + a.dst.co + c * 8)) = o;
    }
    if constexpr (BF) {
        if (a.upsum.p) {
            // fused SSDN_OP_UPSUM_BWD for the channels below upsum_c: 2x2 sums (scan order, fp32) of the bf16 values in the transposed tile,
            // times LeakyReLU'(upsum_mask), to the half-resolution tensor: 4 x 8 pooled pixels of this half
            const int ucp = a.upsum_c >> 3;
            for (int e = tid; e < 32 * ucp; e += C16_THREADS) {
                const int pp_l = e / ucp, c = e - pp_l * ucp;
                const int pi = pp_l >> 3, pj = pp_l & 7;
                const long long pp = ((long long)img * 8 + half * 4 + pi) * 8 + pj;
                const u32x4_t um = *reinterpret_cast<const u32x4_t*>((const h16*)a.upsum_mask.p + (pp * a.upsum_mask.cs + a.upsum_mask.co + c * 8));
                float sum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    const u32x4_t o = *reinterpret_cast<const u32x4_t*>(ot + ((2 * pi + (q4 >> 1)) * 16 + 2 * pj + (q4 & 1)) * OSTR + c * 16);
#pragma unroll
                    for (int k = 0; k < 4; ++k) { sum[2 * k] += bf_lo(o[k]); sum[2 * k + 1] += bf_hi(o[k]); }
                }
                u32x4_t r;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    r[k] = pack_bf16x2(sum[2 * k] * lrelu_grad(f16_lo(um[k])), sum[2 * k + 1] * lrelu_grad(f16_hi(um[k])));
                *reinterpret_cast<u32x4_t*>((h16*)a.upsum.p + (pp * a.upsum.cs + a.upsum.co + c * 8)) = r;
            }
        }
    }
}

static C16Aux c16_aux(const ssdn_conv_args* a) {
    C16Aux x;
    int mny = 0, mnx = 0;
    for (int t = 0; t < a->ntaps; ++t) {
        mny = a->dy[t] < mny ? a->dy[t] : mny;
        mnx = a->dx[t] < mnx ? a->dx[t] : mnx;
    }
    x.padT = -mny; x.padL = -mnx;
    x.pa = a->c0 > 0 ? a->c0 / 8 + 1 : 0;
    x.pb = a->c1 > 0 ? a->c1 / 8 + 1 : 0;
    x.mg_pa = c16_magic((unsigned)x.pa); x.mg_pb = c16_magic((unsigned)x.pb);
    x.rega = (C16_NP * x.pa * 16 + 1023) & ~1023;
    x.tile_bytes = x.rega + ((C16_NP * x.pb * 16 + 1023) & ~1023);
    return x;
}

static int c16_lds(const ssdn_conv_args* a) {
    const int mt = a->Mpad / 32;
    const int slot = ((mt * 32 * C16_WROW + 255) / 256) * 4 * 1024;
    const int main_b = c16_aux(a).tile_bytes + c16_ring(mt, a->bf16 != 0) * slot;
    const int epi_b = 128 * (mt * 64 + 16) + mt * 32 * 4;
    return main_b > epi_b ? main_b : epi_b;
}

// The shape class: what decode_block_3.0 / 3.2 of the blind-spot (and the plain) network are at 16x16 pixels -- a 3x3 layer on whole
// 16x16 images in 48-channel chunks, 96 or 144 input channels in at most two sources of whole chunks, 96 output channels (or the 144
// of decode_block_3.0's data gradient), 16-bit output, and of the fused outputs only the ones the kernel's epilogue has.
bool conv16_shape_ok(const ssdn_conv_args* a) {
    if (a->ntaps != 9 || a->H != 16 || a->W != 16 || a->ltw != 4 || a->lth != 4 || a->ltn != 0 || a->kc != 48) return false;
    if ((a->Ktot != 96 && a->Ktot != 144) || a->c0 % 48 || a->c1 % 48 || a->c0 + a->c1 != a->Ktot) return false;
    if (a->up0 && a->c0 == 0) return false;
    if (!((a->Mpad == 96 && a->M == 96) || (a->Mpad == 160 && a->M == 144 && a->bf16))) return false;
    if (a->dst32 || a->pool.p || a->urot.p || a->unrot.p || a->urot_smask || a->unrot_smask || a->sign_out || a->mask_sign || a->upsum_mask_sign) return false;
    if (a->upsum.p && (!a->bf16 || (a->upsum_c & 7) || a->upsum_c <= 0 || a->upsum_c > a->M)) return false;
    int mny = 0, mxy = 0, mnx = 0, mxx = 0;
    for (int t = 0; t < 9; ++t) {
        mny = a->dy[t] < mny ? a->dy[t] : mny; mxy = a->dy[t] > mxy ? a->dy[t] : mxy;
        mnx = a->dx[t] < mnx ? a->dx[t] : mnx; mxx = a->dx[t] > mxx ? a->dx[t] : mxx;
    }
    return mxy - mny == C16_HH - 8 && mxx - mnx == C16_HW - 16;          // the halo of an 8-row half is 10 x 18 pixels
}

int conv16_lds_bytes(const ssdn_conv_args* a) { return c16_lds(a); }

template <int MT, bool BF>
static int c16_launch(const ssdn_conv_args* a, hipStream_t s) {
    const size_t lds = (size_t)c16_lds(a);
    if (lds > 160 * 1024) return ssdn_set_error("conv16: needs %zu B of LDS (> 160 KiB)", lds);
    static bool attr_set_dev[SSDN_MAX_DEVICES_ATTR] = {};
    bool& attr_set = attr_set_dev[ssdn_current_device_slot()];   // (function attributes are per device)
    if (!attr_set) {
        SSDN_CHECK_HIP(hipFuncSetAttribute((const void*)k_conv16<MT, BF>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr_set = true;
    }
    const double px = (double)a->N * a->H * a->W;
    const int kreal = a->kreal > 0 ? a->kreal : a->Ktot;
    const double flops = 2.0 * px * a->M * kreal * a->ntaps;
    const double bytes = px * (a->c0 * 2.0 / (a->up0 ? 4.0 : 1.0) + a->c1 * 2.0) + px * a->M * 2.0;
    const int grid = ((2 * a->N + 15) / 16) * 16;
    prof_begin(SSDN_PROF_CONV_MT1, s);                     // (the launches it replaces were k_conv<1, ...>)
    SSDN_LAUNCH((k_conv16<MT, BF>), dim3(grid), dim3(C16_THREADS), lds, s, *a, c16_aux(a));
    prof_end(SSDN_PROF_CONV_MT1, s, flops, bytes);
    SSDN_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_conv16(const ssdn_conv_args* a, hipStream_t s) {
    if (!conv16_shape_ok(a)) return ssdn_set_error("conv16: not a launch of its shape class");
    if (a->Mpad == 160) return c16_launch<5, true>(a, s);
    return a->bf16 ? c16_launch<3, true>(a, s) : c16_launch<3, false>(a, s);
}
