// tail_fused.hip -- the closing slab reductions, Adam and the re-pack of a training step as ONE launch (k_tail_fused).
// A single-GPU step ends with the last gradient bucket's SSDN_OP_WREDUCE run, SSDN_OP_ADAM and the layers' SSDN_OP_WPACK ops on one
// stream with nothing beside them: three latency-bound launches (stage 1, stage 2, k_adam_pack) that hand each other a group partial and
// the reduced gradient through memory.  Here the block that owns a weight tile sums the tile straight from the slabs -- in the order the
// two-stage kernels use, so the bit pattern is theirs --, stores the gradient (the flat gradient stays an output of the step) and feeds
// the same value to the Adam element and the shadow stores of adam_pack.h.  The slabs are only READ (stage 1 overwrites the first slab
// of every group): the launch is repeatable.
// Work split: k_adam_pack's -- a block owns one tile of one layer (AP_TM output channels x AP_TK input channels x all taps) or 1024
// elements of a stretch of the Adam range without shadows -- except that a tile with more than TF_SPLIT_BYTES of slab data behind it
// is cut into four quarters along the input channels (a 96 -> 96 3x3 layer has 24 tiles and may have 60 slabs of 332 KB: 850 KB behind
// one block, while the chip-wide average is 250 KB per CU).  Blocks are dispatched heaviest first.
#include "adam_pack.h"
#include <cstring>
#include <mutex>
#include <vector>
#include <algorithm>

#define TF_GROUP 32               // slabs per group of the two-stage summation order (WR_GROUP of elementwise.hip)
#define TF_MAX_GROUPS 8           // at most 256 slabs per entry
#define TF_TKQ (AP_TK / 4)        // channels of a quarter tile
#ifndef TF_SPLIT_BYTES
#define TF_SPLIT_BYTES (256 << 10)
#endif
#ifndef TF_DEPTH
#define TF_DEPTH 8                // slab loads of a thread in flight
#endif
#define TF_STRETCH (EW_BLOCK * 4) // elements of a stretch block

// bias gradients of a pending entry that a stretch block meets: elements [start, start + len) of the Adam range
struct TfSeg { long long start; int len, entry; };
// one block of the launch
struct TfBlock {
    int layer;   // >= 0: a tile of re-pack entry `layer`; < 0: a stretch block of stretch -1 - layer
    int tile;    // tile of the layer (row of tiles major) / block of the stretch
    int entry;   // tile: the pending reduction that covers it, or -1 (gradient read from memory); stretch: first bias segment it meets
    int sub;     // tile: -1 whole, 0..3 quarter along the input channels; stretch: number of bias segments it meets
};
// the static part of a run, in device memory, followed by nblocks TfBlock (cached per distinct run)
struct TfTable {
    ssdn_wpack_args e[ADAM_PACK_MAX];
    ssdn_wreduce_args r[WREDUCE_MULTI_MAX];
    TfSeg seg[WREDUCE_MULTI_MAX];
    long long w_off[ADAM_PACK_MAX];             // first element of the layer's weights in the Adam range
    long long gap_start[ADAM_PACK_MAX + 2];     // stretches of the range without shadows: [gap_start, gap_end)
    long long gap_end[ADAM_PACK_MAX + 2];
    int tiles_k[ADAM_PACK_MAX];                 // 48-channel tiles per row of tiles
    int n, nent, ngaps, nseg, nblocks, pad[3];
};
typedef const __attribute__((address_space(4))) TfTable* TfTableC;
typedef const __attribute__((address_space(4))) TfBlock* TfBlockC;

// The two-stage order for one float4 column of one slab group: a chain of fp32 adds from +0.0f over the group's slabs in ascending
// order, TF_DEPTH 16-byte loads in flight (a short last round is predicated, not a loop of dependent single loads).
// p: the column in slab 0; st4: slab stride in float4.
static __device__ __forceinline__ float4 tf_chain(const float4* p, long long st4, int s0, int s1) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s = s0; s < s1; s += TF_DEPTH) {
        float4 v[TF_DEPTH];
#pragma unroll
        for (int u = 0; u < TF_DEPTH; ++u)
            if (s + u < s1) v[u] = p[(long long)(s + u) * st4];
#pragma unroll
        for (int u = 0; u < TF_DEPTH; ++u)
            if (s + u < s1) { acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w; }
    }
    return acc;
}
// gradient of a tile's element from the group sums parked in LDS: the chain from +0.0f over the group partials in ascending order
// (one group: the chain over the slabs itself), times inv_scale with one rounding; stored to the flat gradient, handed to Adam
struct TfGradFromSlabs {
    float* gw;          // the Adam range's gradient (the entry's gw block lies in it at the same offsets as its weights in p)
    const float* psum;  // [groups][tile slots]
    int groups, gstride;
    float inv;
    __device__ __forceinline__ float operator()(long long idx, bool ok, int slot) const {
        if (!ok) return 0.f;
        float sum = psum[slot];
        if (groups > 1) {
            sum = 0.f + sum;
            for (int g = 1; g < groups; ++g) sum += psum[g * gstride + slot];
        }
        const float gr = __fmul_rn(sum, inv);
        gw[idx] = gr;
        return gr;
    }
};
// one tile (TK = AP_TK) or quarter tile (TK = TF_TKQ) at output channel mo0, input channel k0 of layer j
template <int NT, int TK>
static __device__ __forceinline__ void tf_tile(const TfTable& t, const ssdn_adam_args& a, int j, int ent, int mo0, int k0, float* lds,
                                               float inv_bc2s, float step) {
    const ssdn_wpack_args& w = t.e[j];
    if (ent < 0) adam_pack_update<NT, TK>(a, w, t.w_off[j], mo0, k0, lds, inv_bc2s, step, ApGradFromMemory{a.g});
    else {
        const ssdn_wreduce_args& r = t.r[ent];
        constexpr int K4 = TK / 4, F = NT * AP_TM * K4, SLOTS = NT * AP_TM * (TK + 1);
        const int groups = (r.nslabs + TF_GROUP - 1) / TF_GROUP;
        const int ml0 = mo0 - r.m_off, kl0 = k0 - r.c_off;      // the tile's corner inside the entry's block (host: both >= 0)
        const long long st4 = ((long long)r.ntaps * r.Mpad * r.Kpad) >> 2;
        for (int item = threadIdx.x; item < groups * F; item += EW_BLOCK) {
            const int g = item / F, f = item - g * F;
            const int row = f / K4, k4 = f - row * K4;
            const int tp = row / AP_TM, mo = row - tp * AP_TM;
            const int ml = ml0 + mo, kl = kl0 + 4 * k4;
            if (ml >= r.M || kl >= r.cin) continue;             // (slots of no element: never read)
            const float4* p = reinterpret_cast<const float4*>(r.slab + ((long long)tp * r.Mpad + ml) * r.Kpad + kl);
            const int s0 = g * TF_GROUP, s1 = s0 + TF_GROUP < r.nslabs ? s0 + TF_GROUP : r.nslabs;
            const float4 acc = tf_chain(p, st4, s0, s1);
            float* d = lds + g * SLOTS + ap_slot<TK>(tp, mo, 4 * k4);
            d[0] = acc.x; d[1] = acc.y; d[2] = acc.z; d[3] = acc.w;
        }
        __syncthreads();
        // (the updated tile is parked over group 0's sums: a thread reads every group's sum of a slot before it writes that slot,
        //  and no other thread touches the slot)
        const TfGradFromSlabs gsrc{const_cast<float*>(a.g), lds, groups, SLOTS, r.inv_scale ? *r.inv_scale : 1.f};
        adam_pack_update<NT, TK>(a, w, t.w_off[j], mo0, k0, lds, inv_bc2s, step, gsrc);
    }
    __syncthreads();
    adam_pack_store<NT, TK>(w, mo0, k0, lds);
}

__global__ __launch_bounds__(EW_BLOCK) void k_tail_fused(const TfTable* __restrict__ tab, const TfBlock* __restrict__ blocks, ssdn_adam_args a) {
    extern __shared__ __attribute__((aligned(16))) float tf_lds[];
    const TfTable& t = *(const TfTable*)(TfTableC)(unsigned long long)tab;
    const TfBlockC bp = (TfBlockC)(unsigned long long)(blocks + blockIdx.x);
    const int layer = bp->layer, tile = bp->tile, ent = bp->entry, sub = bp->sub;
    const float inv_bc2s = 1.f / sqrtf(a.bc2);
    const float step = a.lr / a.bc1;
    if (layer >= 0) {
        const int tk = t.tiles_k[layer];
        const int mo0 = (tile / tk) * AP_TM, k0 = (tile % tk) * AP_TK;
        if (t.e[layer].ntaps == 9) {
            if (sub < 0) tf_tile<9, AP_TK>(t, a, layer, ent, mo0, k0, tf_lds, inv_bc2s, step);
            else tf_tile<9, TF_TKQ>(t, a, layer, ent, mo0, k0 + sub * TF_TKQ, tf_lds, inv_bc2s, step);
        } else tf_tile<1, AP_TK>(t, a, layer, ent, mo0, k0, tf_lds, inv_bc2s, step);
    } else {
        const int gp = -1 - layer;
        const long long first = t.gap_start[gp] + (long long)tile * TF_STRETCH + threadIdx.x;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long i = first + u * EW_BLOCK;
            if (i >= t.gap_end[gp]) continue;
            int e = -1, m = 0;
            for (int q = 0; q < sub; ++q) {
                const long long d = i - t.seg[ent + q].start;
                if (d >= 0 && d < t.seg[ent + q].len) { e = t.seg[ent + q].entry; m = (int)d; }
            }
            if (e < 0) { adam_elem(a, i, inv_bc2s, step); continue; }
            // bias gradient of a pending entry: ONE chain over all slabs in index order, 16 loads in flight (as wreduce_final)
            const ssdn_wreduce_args& r = t.r[e];
            float acc = 0.f;
            int s = 0;
            for (; s + 16 <= r.nslabs; s += 16) {
                float v[16];
#pragma unroll
                for (int x = 0; x < 16; ++x) v[x] = r.bslab[(long long)(s + x) * r.Mpad + m];
#pragma unroll
                for (int x = 0; x < 16; ++x) acc += v[x];
            }
            for (; s < r.nslabs; ++s) acc += r.bslab[(long long)s * r.Mpad + m];
            const float gr = __fmul_rn(acc, r.inv_scale ? *r.inv_scale : 1.f);
            const_cast<float*>(a.g)[i] = gr;
            adam_apply(a, i, AdamIn{gr, a.m[i], a.v[i], a.p[i]}, inv_bc2s, step);
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
namespace {
struct TfPlan {
    TfTable t;
    std::vector<TfBlock> blocks;
    size_t lds;
};
struct TfCache {
    std::vector<char> key;      // the run's argument structs (Adam: pointers and length only), byte for byte
    char* dev;                  // TfTable + blocks; nullptr: the run is not fusable
    int device, nblocks;
    size_t lds;
};
std::vector<TfCache> g_tf_cache;
std::mutex g_tf_mutex;
}

// Can the run [reductions wr[0..nw)] [Adam a] [re-packs wp[0..np)] be ONE launch?  (adam_pack_fusable(a, wp, np) holds.)  Fills `out`.
// Refused, i.e. left to the present kernels:
//   - accumulate != 0 (the epilogue would read the old gradient) and tapblock = 1 (channel-block slabs of the 1x1 head layers: their
//     reductions run on the side lane in every BASELINE plan, never in front of Adam);
//   - an entry whose gw is not the gradient of one of the re-packed layers at the layer's own place in the Adam range, or whose gb
//     block does not lie inside ONE stretch without shadows: every element then belongs to exactly one block of the launch;
//   - an entry whose block is not made of whole tiles: m_off and c_off multiples of AP_TM / AP_TK, the far edges multiples too or the
//     layer's last channel -- one tile then belongs to at most one entry;
//   - overlapping entries, more entries or layers than the tables hold, more than TF_MAX_GROUPS groups of slabs, Kpad & 3.
static bool tail_fusable(const ssdn_wreduce_args* const* wr, int nw, const ssdn_adam_args* a, const ssdn_wpack_args* const* wp, int np, TfPlan* out) {
    if (nw < 1 || nw > WREDUCE_MULTI_MAX || np < 1 || np > ADAM_PACK_MAX || !a->g || !a->p) return false;
    TfTable& t = out->t;
    memset(&t, 0, sizeof(t));
    t.n = np; t.nent = nw;
    // layers and stretches: launch_adam_pack's split
    long long pos = 0;
    int ng = 0;
    auto gap = [&](long long start, long long end) {
        if (end <= start) return;
        t.gap_start[ng] = start; t.gap_end[ng] = end;
        ++ng;
    };
    for (int i = 0; i < np; ++i) {
        t.e[i] = *wp[i];
        t.w_off[i] = wp[i]->w - a->p;
        t.tiles_k[i] = (wp[i]->cin + AP_TK - 1) / AP_TK;
        gap(pos, t.w_off[i]);
        pos = t.w_off[i] + (long long)wp[i]->M * wp[i]->cin * wp[i]->ntaps;
    }
    gap(pos, a->n);
    t.ngaps = ng;
    // entries
    int layer_of[WREDUCE_MULTI_MAX];
    for (int i = 0; i < nw; ++i) {
        const ssdn_wreduce_args* r = wr[i];
        if (r->accumulate || r->tapblock || (r->Kpad & 3) || r->nslabs < 1 || r->nslabs > TF_GROUP * TF_MAX_GROUPS) return false;
        if (!r->slab || !r->gw || r->M < 1 || r->cin < 1 || r->M > r->Mpad || r->cin > r->Kpad || r->m_off < 0 || r->c_off < 0) return false;
        int j = -1;
        for (int l = 0; l < np; ++l)
            if (r->gw == a->g + t.w_off[l]) j = l;
        if (j < 0) return false;
        const ssdn_wpack_args* w = wp[j];
        if (r->ntaps != w->ntaps || r->cin_full != w->cin) return false;
        const int m1 = r->m_off + r->M, c1 = r->c_off + r->cin;
        if (m1 > w->M || c1 > w->cin) return false;
        if (r->m_off % AP_TM || (m1 % AP_TM && m1 != w->M) || r->c_off % AP_TK || (c1 % AP_TK && c1 != w->cin)) return false;
        for (int q = 0; q < i; ++q)
            if (layer_of[q] == j && r->m_off < wr[q]->m_off + wr[q]->M && wr[q]->m_off < m1 && r->c_off < wr[q]->c_off + wr[q]->cin && wr[q]->c_off < c1)
                return false;
        layer_of[i] = j;
        t.r[i] = *r;
        if (r->gb) {
            if (!r->bslab) return false;
            const long long start = (r->gb - a->g) + r->m_off;
            bool inside = false;
            for (int g = 0; g < ng; ++g) inside = inside || (start >= t.gap_start[g] && start + r->M <= t.gap_end[g]);
            if (r->gb < a->g || !inside) return false;
            for (int q = 0; q < t.nseg; ++q)
                if (start < t.seg[q].start + t.seg[q].len && t.seg[q].start < start + r->M) return false;
            t.seg[t.nseg++] = TfSeg{start, r->M, i};
        }
    }
    std::stable_sort(t.seg, t.seg + t.nseg, [](const TfSeg& x, const TfSeg& y) { return x.start < y.start; });
    // blocks: {cost, block}; the quarters of heavy tiles first, eight tiles at a time with the quarters of a tile eight blocks apart
    // (blocks are dealt round-robin over the eight XCDs: the quarters share their 128-byte lines of the slabs through one L2), then
    // everything else, heaviest first (stable: deterministic tables)
    struct Unit { long long cost; TfBlock b; };
    std::vector<Unit> heavy, rest;
    size_t lds = 0;
    for (int j = 0; j < np; ++j) {
        const ssdn_wpack_args* w = wp[j];
        const int tm = (w->M + AP_TM - 1) / AP_TM, tk = t.tiles_k[j];
        for (int tile = 0; tile < tm * tk; ++tile) {
            const int mo0 = (tile / tk) * AP_TM, k0 = (tile % tk) * AP_TK;
            int ent = -1;
            for (int i = 0; i < nw; ++i)
                if (layer_of[i] == j && mo0 >= wr[i]->m_off && mo0 < wr[i]->m_off + wr[i]->M && k0 >= wr[i]->c_off && k0 < wr[i]->c_off + wr[i]->cin) ent = i;
            const int kw = std::min(AP_TK, w->cin - k0);        // channels of the tile
            const long long elems = (long long)w->ntaps * AP_TM * kw;
            const long long bytes = elems * 16 + (ent >= 0 ? elems * 4 * wr[ent]->nslabs : 0);
            const int groups = ent >= 0 ? (wr[ent]->nslabs + TF_GROUP - 1) / TF_GROUP : 1;
            if (ent >= 0 && w->ntaps == 9 && (long long)9 * AP_TM * AP_TK * 4 * wr[ent]->nslabs > TF_SPLIT_BYTES) {
                for (int sub = 0; sub * TF_TKQ < kw; ++sub) heavy.push_back({bytes / ((kw + TF_TKQ - 1) / TF_TKQ), TfBlock{j, tile, ent, sub}});
                lds = std::max(lds, (size_t)groups * 9 * AP_TM * (TF_TKQ + 1) * 4);
            } else {
                rest.push_back({bytes, TfBlock{j, tile, ent, -1}});
                lds = std::max(lds, (size_t)groups * w->ntaps * AP_TM * (AP_TK + 1) * 4);
            }
        }
    }
    for (int g = 0; g < ng; ++g) {
        const int nb = (int)((t.gap_end[g] - t.gap_start[g] + TF_STRETCH - 1) / TF_STRETCH);
        for (int b = 0; b < nb; ++b) {
            const long long lo = t.gap_start[g] + (long long)b * TF_STRETCH, hi = std::min(lo + TF_STRETCH, t.gap_end[g]);
            int first = -1, cnt = 0;
            long long bytes = (hi - lo) * 16;
            for (int q = 0; q < t.nseg; ++q)
                if (t.seg[q].start < hi && lo < t.seg[q].start + t.seg[q].len) {
                    if (first < 0) first = q;
                    cnt = q - first + 1;
                    bytes += (long long)t.seg[q].len * 4 * wr[t.seg[q].entry]->nslabs;
                }
            rest.push_back({bytes, TfBlock{-1 - g, b, first < 0 ? 0 : first, cnt}});
        }
    }
    // (the quarters of one tile stand next to each other in `heavy`, and cost the same: a stable sort keeps them together)
    std::stable_sort(heavy.begin(), heavy.end(), [](const Unit& x, const Unit& y) { return x.cost > y.cost; });
    std::vector<TfBlock>& blocks = out->blocks;
    blocks.clear();
    size_t h = 0;
    while (h < heavy.size()) {
        // the next (up to) eight tiles
        size_t tiles_first[9];
        int nt = 0;
        size_t q = h;
        while (q < heavy.size() && nt < 8) {
            tiles_first[nt++] = q;
            const TfBlock& b0 = heavy[q].b;
            while (q < heavy.size() && heavy[q].b.layer == b0.layer && heavy[q].b.tile == b0.tile) ++q;
        }
        tiles_first[nt] = q;
        for (int sub = 0; sub < 4; ++sub)
            for (int k = 0; k < nt; ++k)
                if (tiles_first[k] + sub < tiles_first[k + 1]) blocks.push_back(heavy[tiles_first[k] + sub].b);
        h = q;
    }
    std::stable_sort(rest.begin(), rest.end(), [](const Unit& x, const Unit& y) { return x.cost > y.cost; });
    for (const Unit& u : rest) blocks.push_back(u.b);
    t.nblocks = (int)blocks.size();
    out->lds = lds;
    return t.nblocks > 0 && lds <= 64 * 1024;
}

// the run's cached tables (built on first sight); dev == nullptr: the run is not fusable
static int tf_lookup(const ssdn_wreduce_args* const* wr, int nw, const ssdn_adam_args* a, const ssdn_wpack_args* const* wp, int np,
                     char** dtab, int* nblocks, size_t* lds) {
    *dtab = nullptr;
    if (nw < 1 || nw > WREDUCE_MULTI_MAX || np < 1 || np > ADAM_PACK_MAX) return 0;
    // key: everything the tables are made from (lr, the bias corrections and gscale change every step and travel as kernel arguments)
    struct { const void *p, *g, *m, *v; long long n; int nw, np; } head = {a->p, a->g, a->m, a->v, (long long)a->n, nw, np};
    std::vector<char> key(sizeof(head) + (size_t)nw * sizeof(ssdn_wreduce_args) + (size_t)np * sizeof(ssdn_wpack_args));
    memcpy(key.data(), &head, sizeof(head));
    for (int i = 0; i < nw; ++i) memcpy(key.data() + sizeof(head) + (size_t)i * sizeof(ssdn_wreduce_args), wr[i], sizeof(ssdn_wreduce_args));
    for (int i = 0; i < np; ++i)
        memcpy(key.data() + sizeof(head) + (size_t)nw * sizeof(ssdn_wreduce_args) + (size_t)i * sizeof(ssdn_wpack_args), wp[i], sizeof(ssdn_wpack_args));
    int dev = 0;
    SSDN_CHECK_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(g_tf_mutex);
    const TfCache* hit = nullptr;
    for (const TfCache& c : g_tf_cache)
        if (c.device == dev && c.key.size() == key.size() && !memcmp(c.key.data(), key.data(), key.size())) { hit = &c; break; }
    if (!hit) {
        if (g_tf_cache.size() >= 64) {
            SSDN_CHECK_HIP(hipDeviceSynchronize());
            if (g_tf_cache.front().dev) SSDN_CHECK_HIP(hipFree(g_tf_cache.front().dev));
            g_tf_cache.erase(g_tf_cache.begin());
        }
        TfPlan plan;
        TfCache c{key, nullptr, dev, 0, 0};
        if (tail_fusable(wr, nw, a, wp, np, &plan)) {
            const size_t bytes = sizeof(TfTable) + sizeof(TfBlock) * plan.blocks.size();
            std::vector<char> host(bytes);
            memcpy(host.data(), &plan.t, sizeof(TfTable));
            memcpy(host.data() + sizeof(TfTable), plan.blocks.data(), sizeof(TfBlock) * plan.blocks.size());
            SSDN_CHECK_HIP(hipMalloc((void**)&c.dev, bytes));
            SSDN_CHECK_HIP(hipMemcpy(c.dev, host.data(), bytes, hipMemcpyHostToDevice));
            c.nblocks = plan.t.nblocks;
            c.lds = plan.lds;
        }
        g_tf_cache.push_back(c);
        hit = &g_tf_cache.back();
    }
    *dtab = hit->dev; *nblocks = hit->nblocks; *lds = hit->lds;
    return 0;
}
// -> 1: launch_tail_fused will run this run as one launch; 0: it is left to the present kernels; < 0: error
int tail_fused_ok(const ssdn_wreduce_args* const* wr, int nw, const ssdn_adam_args* a, const ssdn_wpack_args* const* wp, int np) {
    char* dtab;
    int nblocks;
    size_t lds;
    const int rc = tf_lookup(wr, nw, a, wp, np, &dtab, &nblocks, &lds);
    return rc ? rc : (dtab ? 1 : 0);
}
int launch_tail_fused(const ssdn_wreduce_args* const* wr, int nw, const ssdn_adam_args* a, const ssdn_wpack_args* const* wp, int np, hipStream_t s) {
    char* dtab;
    int nblocks;
    size_t lds;
    const int rc = tf_lookup(wr, nw, a, wp, np, &dtab, &nblocks, &lds);
    if (rc) return rc;
    if (!dtab) return ssdn_set_error("tail_fused: the run is not fusable");
    SSDN_LAUNCH(k_tail_fused, dim3((unsigned)nblocks), dim3(EW_BLOCK), lds, s, (const TfTable*)dtab, (const TfBlock*)(dtab + sizeof(TfTable)), *a);
    return 0;
}
