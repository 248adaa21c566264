"""TEST INFRASTRUCTURE -- references for the optimiser side of a training step: SSDN_OP_WREDUCE, SSDN_OP_ADAM, SSDN_OP_WPACK and the fused
k_adam_pack launch.  CPU only (numpy + torch on the CPU), written from the words of include/ssdn_hip.h; nothing here imports ssdn.hip or
oracle/interp.py.  tests/test_optim_ref_cpu.py checks these references against each other, tests/test_hip_optimiser.py holds the device
to them.

    adam_ref64     the header's formula in float64 on the op's fp32 argument values, with per-element rounding bounds
    adam_model32   a numpy float32 model of the kernel's operation order (diagnostic: it is NOT asserted bit-equal to the device)
    wreduce_ref    float64 sums with a bound, and an exact fp32 model of the documented summation order
    wpack_ref      the four 16-bit weight shadows wf / wd / wfc / wdc
"""
from __future__ import annotations

from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import torch

U = 2.0 ** -24            # unit roundoff of fp32 (round to nearest)
TINY = 2.0 ** -149        # spacing of the fp32 subnormals
FACTOR = 2.0              # what the GPU tests allow on top of the first-order bounds below (second-order terms, 1/sqrtf(bc2))


# ---- SSDN_OP_ADAM ---------------------------------------------------------------------------------------------------------------------
def adam_args(lr, step, gscale, b1=0.9, b2=0.99, eps=1e-8):
    """the fp32 numbers ssdn_adam_args carries for optimiser step `step` (the host computes bc = 1 - beta^step in double and the
    struct rounds every field to fp32 once)"""
    f = np.float32
    return SimpleNamespace(lr=f(lr), b1=f(b1), b2=f(b2), eps=f(eps), bc1=f(1.0 - b1 ** step), bc2=f(1.0 - b2 ** step), gscale=f(gscale))


def adam_inputs(n, seed, zero_moments=False):
    """-> p, g, m, v (numpy float32 [n]) in which every term of the update is visible:
    |g|, |m| log-uniform in [1e-12, 1e2] with independent signs (m' cancels), v log-uniform in [1e-24, 1e4] (a share of the elements has
    sqrt(v')/sqrt(bc2) < 10 eps: the regime that pins where eps sits), p = +-U(0,1) 10^U(-6,0) (the update is not swallowed by p's ulp)."""
    gen = torch.Generator().manual_seed(seed)

    def logu(lo, hi):
        return 10.0 ** (lo + (hi - lo) * torch.rand(n, generator=gen, dtype=torch.float64))

    def sign():
        return torch.randint(0, 2, (n,), generator=gen).double() * 2 - 1
    g = sign() * logu(-12, 2)
    m = sign() * logu(-12, 2)
    v = logu(-24, 4)
    p = sign() * torch.rand(n, generator=gen, dtype=torch.float64) * logu(-6, 0)
    if zero_moments:
        m, v = torch.zeros_like(m), torch.zeros_like(v)
    return tuple(x.float().numpy() for x in (p, g, m, v))


def adam_ref64(p, g, m, v, args):
    """SSDN_OP_ADAM in float64:  G = g gscale,  m' = b1 m + (1-b1) G,  v' = b2 v + (1-b2) G^2,  den = sqrt(v')/sqrt(bc2) + eps,
    q = lr/bc1 m'/den,  p' = p - q, on the fp32 argument values widened to float64 (1 - b1 and 1 - b2 are then exact, and so are the
    kernel's 1.f - b1 and 1.f - b2: both betas lie in [0.5, 1]).

    -> dict(m, v, p, E_m, E_v, E_p): the float64 results and first-order bounds on |fp32 result - float64 result|, u = 2^-24.  The count
    follows adam_apply (csrc/elementwise.hip), each rounding charged to the ADDENDS it acts on, never to the (possibly cancelling) result:

      g~ = fl(g gscale)                                  1 rounding: relative u on G
      m' = fma(b1, m, fl((1-b1) g~))                     the product: u more on (1-b1) G, 2u in all; the fma rounds m' once, and
                                                         |m'| <= |b1 m| + (1-b1)|G|
           E_m = u (|b1 m| + 3 (1-b1)|G|)
      v' = fma(b2, v, fl(fl((1-b2) g~) g~))              G^2 carries 2u from g~, the two products u each: 4u on (1-b2) G^2; the fma
                                                         rounds v' >= 0 once
           E_v = u (v' + 4 (1-b2) G^2)
      den = fma(sqrtf(v'), inv_bc2s, eps)                relative to den (eps is exact and only shrinks the share):
                                                         E_v / v' <= 5u through the square root: 2.5u; sqrtf: u; the fma: u   -> 4.5u
                                                         (inv_bc2s = 1.f / sqrtf(bc2) has two more roundings: left to FACTOR)
      q~ = fl(fl(step m') / den), step = fl(lr / bc1)    3 roundings                                                          -> 3u
      p' = fl(p - q~)                                    u |p'|
           E_p = u |p'| + 10 u |q| + (lr/bc1) E_m / den  (7.5u counted, 9.5u with inv_bc2s: 10u; the last term is m's own error)
    """
    f64 = lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)      # noqa: E731
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    lr, b1, b2, eps, bc1, bc2, gs = (float(np.float32(getattr(args, k))) for k in ("lr", "b1", "b2", "eps", "bc1", "bc2", "gscale"))
    G = g * gs
    m1 = b1 * m + (1.0 - b1) * G
    v1 = b2 * v + (1.0 - b2) * G * G
    den = np.sqrt(v1) / np.sqrt(bc2) + eps
    q = lr / bc1 * m1 / den
    p1 = p - q
    E_m = U * (np.abs(b1 * m) + 3.0 * (1.0 - b1) * np.abs(G))
    E_v = U * (v1 + 4.0 * (1.0 - b2) * G * G)
    E_p = U * np.abs(p1) + 10.0 * U * np.abs(q) + (lr / bc1) * E_m / den
    return dict(m=m1, v=v1, p=p1, E_m=E_m, E_v=E_v, E_p=E_p)


def _fma32(a, b, c):
    """fmaf modelled as the float64 product (exact: 48 bits) and sum, rounded once more to fp32 -- a double rounding in rare cases"""
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
            + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


def adam_model32(p, g, m, v, args):
    """adam_apply's operation order in numpy float32 -> dict(m, v, p) float32.  Diagnostic only (see _fma32)."""
    f = np.float32
    p, g, m, v = (np.asarray(x, dtype=f) for x in (p, g, m, v))
    lr, b1, b2, eps, bc1, bc2, gs = (f(getattr(args, k)) for k in ("lr", "b1", "b2", "eps", "bc1", "bc2", "gscale"))
    one = f(1.0)
    gt = g * gs
    m1 = _fma32(b1, m, (one - b1) * gt)
    v1 = _fma32(b2, v, ((one - b2) * gt) * gt)
    inv_bc2s = one / np.sqrt(bc2)
    step = lr / bc1
    den = _fma32(np.sqrt(v1), inv_bc2s, eps)
    p1 = p - (step * m1) / den
    assert m1.dtype == f and v1.dtype == f and p1.dtype == f and den.dtype == f
    return dict(m=m1, v=v1, p=p1)


def adam_ratios(got_p, got_m, got_v, ref):
    """worst |got - ref| / (E + TINY / FACTOR) per quantity, over EVERY element -> dict(m, v, p).  The GPU tests assert each <= FACTOR,
    which is |got - ref| <= FACTOR E + TINY; the CPU model stays <= 1."""
    out = {}
    for k, got in (("m", got_m), ("v", got_v), ("p", got_p)):
        err = np.abs(np.asarray(got, dtype=np.float32).astype(np.float64) - ref[k])
        assert np.isfinite(err).all(), k
        out[k] = float((err / (ref["E_" + k] + TINY / FACTOR)).max()) if err.size else 0.0
    return out


# ---- SSDN_OP_WREDUCE --------------------------------------------------------------------------------------------------------------------
WR_GROUP = 32


def _seq_sum32(xs):
    """sequential fp32 adds starting from 0.f: ((0 + x_0) + x_1) + ... ; xs: list of equally shaped float32 CPU tensors"""
    acc = torch.zeros_like(xs[0])
    for x in xs:
        acc = acc + x
    return acc


def wreduce_ref(slab, bslab, args, inv=None, with_bias=True, gw0=None, gb0=None):
    """SSDN_OP_WREDUCE from the header's text.
    slab [nslabs][ntaps][Mpad][Kpad], bslab [nslabs][Mpad]: float32 CPU tensors; args: anything with the integer fields of
    ssdn_wreduce_args (nslabs, ntaps, M, Mpad, Kpad, cin, cin_full, m_off, c_off, tapblock, accumulate); inv: the value behind inv_scale
    (None: NULL = 1); with_bias: gb given; gw0 / gb0: what gw / gb hold before the op (accumulate = 1 adds to it).

    Weights: slabs are summed in groups of 32 in index order, then the group sums in order (one group when nslabs <= 32); every sum is a
    chain of fp32 adds that starts from 0.f.  Bias: ONE chain over all slabs in index order, no groups.  The sum is multiplied by
    inv_scale with one rounding; accumulate = 1 is one more add, fl(old + g).  Element (t, m, k), m < M, of the slab goes to
    gw[m_off + m][c_off + k][t] for k < cin -- tapblock: to input channel c_off + t Kpad + k of a 1x1 layer, t Kpad + k < cin -- and
    bias m to gb[m_off + m].

    -> dict, every array flat in the layout of gw ([m_off + M][cin_full][ntaps], tapblock: [m_off + M][cin_full]) resp. gb ([m_off + M]),
    NaN where the op writes nothing:
        w64, b64      float64: (old +) inv * sum
        w_bound, b_bound   nslabs u sum_s |inv x_s| + u |inv sum| (+ u |result| for the add of accumulate = 1)
        w32, b32      float32: the exact model"""
    a = args
    ns, nt, M, Mpad, Kpad = int(a.nslabs), int(a.ntaps), int(a.M), int(a.Mpad), int(a.Kpad)
    slab = slab.reshape(ns, nt, Mpad, Kpad).float()
    bslab = bslab.reshape(ns, Mpad).float()
    tapblock, acc = bool(a.tapblock), bool(a.accumulate)
    nw = (a.m_off + M) * a.cin_full * (1 if tapblock else nt)
    nb = a.m_off + M
    inv32 = torch.tensor(1.0 if inv is None else inv, dtype=torch.float32)
    inv64 = float(inv32)

    # the sums
    if ns > WR_GROUP:
        groups = [_seq_sum32([slab[s] for s in range(s0, min(s0 + WR_GROUP, ns))]) for s0 in range(0, ns, WR_GROUP)]
        w32 = _seq_sum32(groups)
    else:
        w32 = _seq_sum32([slab[s] for s in range(ns)])
    b32 = _seq_sum32([bslab[s] for s in range(ns)])
    w32, b32 = w32 * inv32, b32 * inv32                                     # one rounding each
    w64, b64 = slab.double().sum(0) * inv64, bslab.double().sum(0) * inv64
    wB = ns * U * slab.double().abs().sum(0) * abs(inv64) + U * w64.abs()
    bB = ns * U * bslab.double().abs().sum(0) * abs(inv64) + U * b64.abs()

    # the scatter
    t, m, k = np.meshgrid(np.arange(nt), np.arange(Mpad), np.arange(Kpad), indexing="ij")
    if tapblock:
        ci = t * Kpad + k
        ok = (m < M) & (ci < a.cin)
        dst = (a.m_off + m) * a.cin_full + a.c_off + ci
    else:
        ok = (m < M) & (k < a.cin)
        dst = ((a.m_off + m) * a.cin_full + a.c_off + k) * nt + t
    ok_t, dst_t = torch.from_numpy(ok.reshape(-1)), torch.from_numpy(dst.reshape(-1))[torch.from_numpy(ok.reshape(-1))]
    assert int(dst_t.max()) < nw and len(torch.unique(dst_t)) == len(dst_t)

    def scatter(vals, n, idx, sel, dtype):
        out = torch.full((n,), float("nan"), dtype=dtype)
        out[idx] = vals.reshape(-1)[sel].to(dtype)
        return out
    out = dict(w32=scatter(w32, nw, dst_t, ok_t, torch.float32), w64=scatter(w64, nw, dst_t, ok_t, torch.float64),
               w_bound=scatter(wB, nw, dst_t, ok_t, torch.float64))
    bsel = torch.arange(Mpad) < M
    bidx = a.m_off + torch.arange(M)
    if with_bias:
        out.update(b32=scatter(b32, nb, bidx, bsel, torch.float32), b64=scatter(b64, nb, bidx, bsel, torch.float64),
                   b_bound=scatter(bB, nb, bidx, bsel, torch.float64))
    else:
        out.update(b32=torch.full((nb,), float("nan")), b64=torch.full((nb,), float("nan"), dtype=torch.float64),
                   b_bound=torch.full((nb,), float("nan"), dtype=torch.float64))
    if acc:
        for key, old in (("w", gw0), ("b", gb0)):
            old = old.reshape(-1).float().cpu()
            out[key + "32"] = old + out[key + "32"]                          # one fp32 add (NaN stays NaN: not written)
            out[key + "64"] = old.double() + out[key + "64"]
            out[key + "_bound"] = out[key + "_bound"] + U * out[key + "64"].abs()
    return out


# ---- SSDN_OP_WPACK ----------------------------------------------------------------------------------------------------------------------
def k_to_cin(Ktot, c0, c1_real):
    """input-channel slot k of the packed K axis -> real input channel, -1: padding.  Slots [0, c0) are source 0, slots [c0, c0 + c1_real)
    the real channels of source 1, numbered on from c0; the rest pads Ktot up to a multiple of 16."""
    return np.array([k if k < c0 else (c0 + (k - c0) if k - c0 < c1_real else -1) for k in range(Ktot)], dtype=np.int64)


@lru_cache(maxsize=None)
def chunk_major_positions(ntaps, rows, K):
    """-> int64 [ntaps][rows][K]: where element (t, row, k) of a row-major [ntaps][rows][K] shadow sits in its chunk-major copy
    (ssdn_conv_args.wc): [tap][chunk][rows][kc], chunks of 48 columns, then one optional chunk of 16; inside a row of a chunk the
    16-byte piece (8 elements) p is stored at piece p ^ ((row >> 3) & 1)."""
    nfull, tail = divmod(K, 48)
    assert tail in (0, 16), "chunk-major copies exist only for K = 48 n or 48 n + 16"
    pos = np.empty((ntaps, rows, K), dtype=np.int64)
    for t in range(ntaps):
        for k in range(K):
            c = min(k // 48, nfull)
            kc = 48 if c < nfull else 16
            kk = k - 48 * c
            r = np.arange(rows)
            piece = (kk // 8) ^ ((r >> 3) & 1)
            pos[t, :, k] = t * rows * K + c * 48 * rows + r * kc + piece * 8 + kk % 8
    pos.setflags(write=False)                # (cached: shared between callers)
    return pos


def chunk_major_undo(flat, ntaps, rows, K):
    """the inverse, written from the STORAGE side: walk the chunk-major buffer element by element and say which (t, row, k) it holds
    -> the row-major [ntaps][rows][K] array"""
    flat = np.asarray(flat).reshape(-1)
    assert flat.size == ntaps * rows * K
    nfull = K // 48
    q = np.arange(flat.size)
    t, r = q // (rows * K), q % (rows * K)
    in_tail = r >= nfull * 48 * rows
    c = np.where(in_tail, nfull, r // (48 * rows))
    kc = np.where(in_tail, K - 48 * nfull, 48)
    r2 = r - c * 48 * rows
    row, within = r2 // kc, r2 % kc
    stored_piece, e = within // 8, within % 8
    k = 48 * c + (stored_piece ^ ((row >> 3) & 1)) * 8 + e
    out = np.empty((ntaps, rows, K), dtype=flat.dtype)
    seen = np.zeros((ntaps, rows, K), dtype=np.int64)
    out[t, row, k] = flat
    np.add.at(seen, (t, row, k), 1)
    assert (seen == 1).all()
    return out


def wpack_ref(W, args, need_d=True, cm_f=False, cm_d=False):
    """SSDN_OP_WPACK from the header's words.  W: float32 [M][cin][ntaps] (numpy or CPU tensor); args: anything with M, cin, ntaps, c0,
    c1_real, Mpad_f, Ktot, Mpad_d, Kd.
        wf[t][m][k] = fp16(W[m][cin(k)][t])   m < M, k a real slot; 0 in the padding        [ntaps][Mpad_f][Ktot]
        wd[t][c][m] = bf16(W[m][cin(c)][t])   c < Ktot a real slot, m < M; 0 elsewhere      [ntaps][Mpad_d][Kd]   (need_d)
        wfc / wdc: the chunk-major copies of wf / wd (chunk_major_positions; cm_f / cm_d)
    both conversions round to nearest even.
    -> dict name -> (values: flat int16 tensor of the 16-bit patterns, real: flat bool tensor, False in the padding)"""
    a = args
    W = np.asarray(W, dtype=np.float32).reshape(a.M, a.cin, a.ntaps)
    kmap = k_to_cin(a.Ktot, a.c0, a.c1_real)
    assert kmap.max() < a.cin
    wf = np.zeros((a.ntaps, a.Mpad_f, a.Ktot), dtype=np.float32)
    rf = np.zeros(wf.shape, dtype=bool)
    for k in range(a.Ktot):
        if kmap[k] >= 0:
            wf[:, :a.M, k] = W[:, kmap[k], :].T
            rf[:, :a.M, k] = True

    def bits(x, dtype):
        return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).view(torch.int16).reshape(-1)

    def chunked(x, real, ntaps, rows, K):
        pos = chunk_major_positions(ntaps, rows, K).reshape(-1)
        assert len(np.unique(pos)) == pos.size == x.size
        y, ry = np.empty(x.size, dtype=x.dtype), np.empty(x.size, dtype=bool)
        y[pos], ry[pos] = x.reshape(-1), real.reshape(-1)
        return y, ry
    out = {"wf": (bits(wf, torch.float16), torch.from_numpy(rf.reshape(-1).copy()))}
    if cm_f:
        y, ry = chunked(wf, rf, a.ntaps, a.Mpad_f, a.Ktot)
        out["wfc"] = (bits(y, torch.float16), torch.from_numpy(ry))
    if need_d:
        wd = np.zeros((a.ntaps, a.Mpad_d, a.Kd), dtype=np.float32)
        rd = np.zeros(wd.shape, dtype=bool)
        for c in range(min(a.Mpad_d, a.Ktot)):
            if kmap[c] >= 0:
                wd[:, c, :a.M] = W[:, kmap[c], :].T
                rd[:, c, :a.M] = True
        out["wd"] = (bits(wd, torch.bfloat16), torch.from_numpy(rd.reshape(-1).copy()))
        if cm_d:
            y, ry = chunked(wd, rd, a.ntaps, a.Mpad_d, a.Kd)
            out["wdc"] = (bits(y, torch.bfloat16), torch.from_numpy(ry))
    return out
