"""Helper (no tests): one hand-made SSDN_OP_WGRAD launch on tensors of its own, its float64 reference, and the case table.

WCase mirrors conv_case.Case for the weight gradient.  dz (bf16) and the source (fp16) are channel windows (co = 8, cs = channels + 16) of
wider NaN-filled tensors, with a NaN-filled guard strip in front of the first and behind the last pixel, so that a stride or offset taken
from the wrong view, or a row read past its end, shows.  slab and bslab are sized as include/ssdn_hip.h says and NaN-filled before every
launch; so is the layer-shaped gw / gb pair SSDN_OP_WREDUCE writes the block into, at a non-zero (m_off, c_off).  device=False builds the
operands and the argument struct without a GPU (the pointers are placeholders): the host queries of the library and the reference need no
more.

Four operand generators; expected() evaluates the header's formula in float64 on the 16-bit operands, the source first rounded to bf16,
round-to-nearest-even ("converted to bf16 while it is staged"):
  ints   dz and source dense in {-2..2}: every product and, with 4 N H W < 2^24, every partial sum in any order is an integer that fp32
         holds exactly -- the comparison is bit equality;
  round  the source holds fp16 values of magnitude [0.25, 2) over the whole 11-bit significand, hashed so that exact ties with an even and
         with an odd kept bit and values that round up into the next binade all occur (the others have their last bit set: all 11
         significant bits in use); dz in {-1, 0, 1}.  After the rounding every term lies on the 2^-9 grid and every partial sum below
         2^14: exact in any order, bit equality.  The only generator that tells round-to-nearest-even from truncation and round-half-up;
  probe  dz is zero except for 1.0 at one pixel per output channel -- image corners, both sides of every tile seam in x and in y, the
         last pixel of a ragged tile, image N - 1, the image seams of a tile that holds several images; the source encodes its own
         position (channel k holds y + 1, x + 1 or n + 1 by k % 3), except for the last 8 channels (where Ktot >= 16), which hold the
         edges of the storage type: fp16 subnormals, +-65504 and -0.  Every output element is then ONE product: the bf16 rounding of the
         source at the pixel tap t reaches from the probe of channel m, or +0 outside the image; explain() decodes the pixel a wrong
         element was read from;
  rand   uniform values, compared within (N H W + nslabs) 2^-23 sum_pixels |dz x| per element, the sum taken in float64: every product is
         exact, each fp32 add errs by at most 2^-24 of the running sum <= sum |terms|, one add per pixel and one per slab; the factor 2
         covers the MFMA's internal 16-term summation, whose per-add rounding is not documented as IEEE.  Nothing in it is measured.

TABLE: the launches, one per kernel variant (see tests/test_wgrad_case_cpu.py for what holds the table to its classes and to the plans)."""
import ctypes as C

import numpy as np
import torch

GENS = ("ints", "round", "probe", "rand")
M_OFF, C_OFF = 5, 3          # where the block sits inside the layer-shaped gradient SSDN_OP_WREDUCE writes
EDGES = (0x0001, 0x03FF, 0x8001, 0x83FF, 0x0200, 0x0004, 0x000C, 0x7BFF, 0xFBFF, 0x8000)     # subnormals (two of them ties), +-65504, -0


def _dev():
    return torch.device("cuda:0")


def _lib():
    from ssdn.hip import lib as L
    return L, L.load()


def taps_of(kind, blocks=1):
    """"B" / "P" / "1x1" -> (taps, coff); blocks > 1: the taps of a 1x1 layer are 96-channel blocks of its input"""
    from ssdn.hip import graph
    if kind == "1x1":
        return [(0, 0)] * blocks, [96 * b for b in range(blocks)]
    return list(graph.TAPS_BLIND if kind == "B" else graph.TAPS_PLAIN), [0] * 9


def bf16_rne(x16):
    """fp16 tensor -> its bf16 rounding (round-to-nearest-even), as float64"""
    return x16.float().to(torch.bfloat16).double()


def bf16_trunc(x16):
    """fp16 tensor -> the bf16 value with the low bits cut off, as float64 (a mutant of the reference)"""
    bits = x16.float().contiguous().view(torch.int32) & ~0xFFFF
    return bits.view(torch.float32).double()


def bf16_bits_rne_numpy(h_bits):
    """independent integer model: uint16 fp16 patterns -> uint16 bf16 patterns, round-to-nearest-even on the fp32 bits"""
    u = h_bits.astype(np.uint16).view(np.float16).astype(np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def probe_pixels(N, H, W, TW, TH, TN):
    """the pixels the probe generator looks through, most telling first, without repeats"""
    px = [(0, 0, 0), (0, 0, W - 1), (0, H - 1, 0), (0, H - 1, W - 1), (N - 1, H - 1, W - 1), (N - 1, H // 2, W // 2)]
    if TN > 1:
        px += [p for s in range(TN, N, TN) for p in ((s, 0, 0), (s - 1, H - 1, W - 1))]      # first image of the next tile / last of this one
        if N > 1:
            px += [(1, 0, 0), (1, H - 1, W - 1)]                                               # second image of the first tile
    xs = [p for s in range(TW, W, TW) for p in ((0, (5 * s + 1) % H, s), (0, (5 * s + 1) % H, s - 1))]
    ys = [p for s in range(TH, H, TH) for p in ((0, s, (3 * s + 2) % W), (0, s - 1, (3 * s + 2) % W))]
    for i in range(max(len(xs), len(ys))):
        px += xs[i:i + 1] + ys[i:i + 1]
    if W % TW or H % TH:          # the last pixel of the ragged tile of every image, and the last real row / column next to it
        px += [(N - 1, H - 1, W - 2), (N - 1, H - 2, W - 1), (0, H // 2, W - 1), (0, H - 1, W // 2)]
    out = []
    for p in px:
        if p not in out:
            out.append(p)
    return out


class WCase:
    """One SSDN_OP_WGRAD launch (and the SSDN_OP_WREDUCE behind it) on tensors of its own.  tile = (ltw, lth, ltn), the logarithms."""

    def __init__(self, taps, coff, c0, c1, up0, N, H, W, M, tile, nslabs, csplit=0, mblocks=1, kreal=0, gen="ints", seed=0, device=True,
                 Kpad=None):
        L, lib = _lib()
        assert gen in GENS and not (c0 and c1)
        self.taps, self.coff, self.c0, self.c1, self.up0 = list(taps), list(coff), c0, c1, bool(up0)
        self.N, self.H, self.W, self.M, self.tile, self.nslabs = N, H, W, M, tuple(tile), nslabs
        self.csplit, self.mblocks, self.kreal, self.gen, self.device = csplit, max(1, mblocks), kreal, gen, device
        self.Ktot, self.Mpad, self.ntaps = c0 + c1, (M + 31) // 32 * 32, len(taps)
        self.Kpad = Kpad or (96 if len(set(coff)) > 1 else (self.Ktot + 31) // 32 * 32)
        self.thin = kreal > 0                      # (the table passes kreal for the rows of k_wgrad_thin only)
        # columns of a tap that are real: the rest of the slab is padding (unspecified values)
        kcs = {min(self.Kpad, self.Ktot - c) for c in self.coff}
        assert len(kcs) == 1
        self.kc = kreal if self.thin else kcs.pop()
        self.tapblock = int(len(set(coff)) > 1)
        self.TW, self.TH, self.TN = (1 << t for t in self.tile)
        self.ntiles = -(-W // self.TW) * -(-H // self.TH) * -(-N // self.TN)
        self.hs, self.ws = (H // 2, W // 2) if up0 else (H, W)
        self.edge_lo = self.Ktot                   # probe: first channel of the storage-edge block (none: Ktot)
        gen_t = torch.Generator().manual_seed(7000 + seed)
        self.dz, self.src = getattr(self, "_gen_" + gen)(gen_t)
        assert self.dz.dtype == torch.bfloat16 and self.src.dtype == torch.float16
        self.keep, self.wides = [], []
        self._expected = {}

        a = L.WgradArgs()
        self.ddz, a.dz = self._view(self.dz)
        self.dsrc, v = self._view(self.src)
        if c0:
            a.src0 = v
        else:
            a.src1 = v
        a.c0, a.c1, a.up0, a.N, a.H, a.W, a.ntaps = c0, c1, int(self.up0), N, H, W, self.ntaps
        for t, (dy, dx) in enumerate(self.taps):
            a.dy[t], a.dx[t], a.coff[t] = dy, dx, self.coff[t]
        a.M, a.Mpad, a.Ktot, a.Kpad, a.nslabs = M, self.Mpad, self.Ktot, self.Kpad, nslabs
        a.ltw, a.lth, a.ltn = self.tile
        a.csplit, a.mblocks, a.kreal, a.mega, a.cost = csplit, mblocks, kreal, 0, 0.0
        self.slab_n = self.mblocks * nslabs * self.ntaps * self.Mpad * self.Kpad
        self.bslab_n = self.mblocks * nslabs * self.Mpad
        # the layer the block belongs to: gw [Mfull][cin_full][ntaps] (OIHW) or, tap blocks, [Mfull][cin_full]
        self.cin = self.Ktot if self.tapblock else self.kc
        self.Mfull, self.cin_full = M_OFF + self.mblocks * M + 2, C_OFF + self.cin + 4
        self.reds = []
        if device:
            self.slab = torch.empty(self.slab_n, device=_dev())
            self.bslab = torch.empty(self.bslab_n, device=_dev())
            self.gw = torch.empty(self.Mfull * self.cin_full * (1 if self.tapblock else self.ntaps), device=_dev())
            self.gb = torch.empty(self.Mfull, device=_dev())
            self.one = torch.ones(1, device=_dev())
            a.slab, a.bslab = self.slab.data_ptr(), self.bslab.data_ptr()
            stride = self.ntaps * self.Mpad * self.Kpad
            for mb in range(self.mblocks):
                self.reds.append(L.WreduceArgs(self.slab.data_ptr() + 4 * mb * nslabs * stride, self.bslab.data_ptr() + 4 * mb * nslabs * self.Mpad,
                                               nslabs, self.ntaps, M, self.Mpad, self.Kpad, self.cin, self.cin_full, M_OFF + mb * M, C_OFF,
                                               self.tapblock, self.gw.data_ptr(), self.gb.data_ptr(), self.one.data_ptr(), 0))
        else:
            a.slab = a.bslab = 0x1000
        self.a = a

    # ---- operands ---------------------------------------------------------------------------------------------------------------
    def _shapes(self):
        return (self.N, self.H, self.W, self.mblocks * self.M), (self.N, self.hs, self.ws, self.Ktot)

    def _gen_ints(self, g):
        sd, ss = self._shapes()
        return (torch.randint(-2, 3, sd, generator=g).to(torch.bfloat16), torch.randint(-2, 3, ss, generator=g).to(torch.float16))

    def _gen_rand(self, g):
        sd, ss = self._shapes()
        return ((torch.rand(sd, generator=g) * 2 - 1).to(torch.bfloat16), (torch.rand(ss, generator=g) * 2 - 1).to(torch.float16))

    def _gen_round(self, g):
        sd, ss = self._shapes()
        sign = torch.randint(0, 2, ss, generator=g)
        exp = torch.randint(13, 16, ss, generator=g)                # 2^-2 .. 2^0: |x| in [0.25, 2)
        man = torch.randint(0, 1024, ss, generator=g) | 1           # all 11 significant bits in use
        kind = torch.randint(0, 8, ss, generator=g)
        man = torch.where(kind == 0, (man & ~0xF) | 0x4, man)       # exact tie, the kept bit even
        man = torch.where(kind == 1, (man & ~0xF) | 0xC, man)       # exact tie, the kept bit odd
        man = torch.where(kind == 2, 0x3FC | (man & 3), man)        # the kept bits all ones and at least half an ulp behind them: up into the next binade
        bits = (sign << 15) | (exp << 10) | man
        src = torch.from_numpy(bits.numpy().astype(np.uint16).view(np.float16).copy())
        return torch.randint(-1, 2, sd, generator=g).to(torch.bfloat16), src

    def _gen_probe(self, g):
        sd, ss = self._shapes()
        N, hs, ws, K = ss
        pos = torch.stack([torch.arange(hs)[None, :, None].expand(N, hs, ws), torch.arange(ws)[None, None, :].expand(N, hs, ws),
                           torch.arange(N)[:, None, None].expand(N, hs, ws)], -1) + 1                 # [N,hs,ws,3] = (y+1, x+1, n+1)
        assert int(pos.max()) <= 256
        src = pos[..., torch.arange(K) % 3].to(torch.float16)
        self.edge_lo = K - 8 if K >= 16 else K
        if self.edge_lo < K:
            idx = (torch.arange(N * hs * ws).reshape(N, hs, ws, 1) * 7 + torch.arange(8)) % len(EDGES)
            e = np.array(EDGES, dtype=np.uint16)[idx.numpy()]
            src[..., self.edge_lo:] = torch.from_numpy(e.view(np.float16).copy())
        self.pixels = probe_pixels(self.N, self.H, self.W, self.TW, self.TH, self.TN)
        dz = torch.zeros(sd)
        self.probe_of = [self.pixels[c % len(self.pixels)] for c in range(sd[-1])]                  # dz channel -> its pixel
        for c, (n, y, x) in enumerate(self.probe_of):
            dz[n, y, x, c] = 1.0
        return dz.to(torch.bfloat16), src

    def seam_pixel(self):
        """(n, y, x): the first pixel right of the first tile seam in x on the row the probe generator looks at"""
        s = self.TW
        assert s < self.W
        return 0, (5 * s + 1) % self.H, s

    def _view(self, t):
        """[N,h,w,C] -> the device tensor [N,h,w,C + 16] that holds it at channel 8 (inside a flat NaN-filled buffer with a guard strip of
        16 pixels at either end), and its ssdn_view"""
        L, _ = _lib()
        cs = t.shape[-1] + 16
        if not self.device:
            return None, L.View(0x100000, cs, 8)
        guard = 16 * cs
        n = t.numel() // t.shape[-1] * cs
        flat = torch.full((n + 2 * guard,), float("nan"), dtype=t.dtype)
        flat[guard:guard + n].view(t.shape[:-1] + (cs,))[..., 8:8 + t.shape[-1]] = t
        d = flat.to(_dev())
        self.keep.append(d)
        self.wides.append((d, guard, n, cs, t.shape[-1]))
        return d, L.View(d.data_ptr() + guard * t.element_size(), cs, 8)

    # ---- the reference ----------------------------------------------------------------------------------------------------------
    def _im2col(self, xb, taps, halo="zero"):
        """xb: the bf16-rounded source, float64 [N,hs,ws,Ktot] -> [N H W, ntaps kc]: the real columns of every tap at every pixel"""
        N, H, W = self.N, self.H, self.W
        x = xb.repeat_interleave(2, 1).repeat_interleave(2, 2) if self.up0 else xb
        xp = torch.zeros(N, H + 4, W + 4, self.Ktot, dtype=torch.float64)
        xp[:, 2:2 + H, 2:2 + W] = x
        if halo == "top":         # (mutant) the rows above the image repeat its first row
            xp[:, :2, 2:2 + W] = x[:, :1]
        cols = [xp[:, 2 + dy:2 + dy + H, 2 + dx:2 + dx + W, c:c + self.kc] for (dy, dx), c in zip(taps, self.coff)]
        return torch.stack(cols, 3).reshape(N * H * W, self.ntaps * self.kc)

    def evaluate(self, mutant=None, dtype=torch.float64, order=None):
        """the header's formula -> (slab sum [mblocks][ntaps][M][kc], bslab sum [mblocks][M], sum |dz x| like the first).
        mutant: one of MUTANTS, a reference that is wrong in that way.  dtype / order: the accumulation type and the pixel order
        ("rev16": chunks of 16 pixels from the last to the first, each added to a running sum) of the fairness checks."""
        dz, src, taps = self.dz.double(), self.src, self.taps
        xb = bf16_trunc(src) if mutant == "trunc" else bf16_rne(src)
        if mutant == "drop":                 # one pixel never summed
            dz = dz.clone()
            dz[self.N - 1, self.H // 2, self.W // 2] = 0
        elif mutant == "seam":               # one seam pixel read from the column left of it
            n, y, x = self.seam_pixel()
            xb = xb.clone()
            xb[n, y, x] = xb[n, y, x - 1]
        elif mutant == "swap_dydx":
            taps = [(dx, dy) for dy, dx in taps]
        elif mutant == "swap_channels":
            xb = xb.clone()
            xb[..., [0, 1]] = xb[..., [1, 0]]
        X = self._im2col(xb, taps, "top" if mutant == "halo" else "zero")
        D = dz.reshape(-1, self.mblocks * self.M)

        def shape(e):
            return e.reshape(self.mblocks, self.M, self.ntaps, self.kc).permute(0, 2, 1, 3).contiguous()
        if dtype == torch.float64 and order is None:
            return shape(D.T @ X) + 0.0, D.sum(0).reshape(self.mblocks, self.M) + 0.0, shape(D.abs().T @ X.abs())
        D, X = D.to(dtype), X.to(dtype)
        if order is None:
            return shape(D.T @ X), D.sum(0).reshape(self.mblocks, self.M), None
        assert order == "rev16"
        e, b = torch.zeros(D.shape[1], X.shape[1], dtype=dtype), torch.zeros(D.shape[1], dtype=dtype)
        for p in range((D.shape[0] - 1) // 16 * 16, -1, -16):
            e = e + D[p:p + 16].T @ X[p:p + 16]
            b = b + D[p:p + 16].sum(0)
        return shape(e), b.reshape(self.mblocks, self.M), None

    def expected(self):
        """evaluate() of the launch as it should be, after asserting what makes the generator's comparison fair (cached)"""
        if not self._expected:
            E, Eb, A = self.evaluate()
            NHW = self.N * self.H * self.W
            if self.gen == "ints":
                assert 4 * NHW < 2 ** 24 and bool((E == E.round()).all()) and bool((Eb == Eb.round()).all())
            elif self.gen == "round":
                bits = torch.from_numpy(self.src.numpy().view(np.uint16).astype(np.int64))
                low, kept, top = bits & 7, (bits >> 3) & 1, (bits >> 3) & 0x7F
                for what, m in (("tie, even", (low == 4) & (kept == 0)), ("tie, odd", (low == 4) & (kept == 1)), ("next binade", (top == 0x7F) & (low >= 4))):
                    assert bool(m.any()), "no source value is a %s case" % what
                a = self.src.float().abs()
                assert float(a.min()) >= 0.25 and float(a.max()) < 2 and bool((bits & 1).bool().any())
                xb = bf16_rne(self.src)
                assert bool((xb * 512 == (xb * 512).round()).all()) and 2 * NHW <= 2 ** 14 and float(A.max()) < 2 ** 14
            elif self.gen == "probe":
                assert bool((self.dz.float().abs().sum((0, 1, 2)) == 1).all())          # one product per output element
                assert torch.equal(E, self.probe_expected())
            self._expected.update(E=E, Eb=Eb, A=A)
        return self._expected["E"], self._expected["Eb"], self._expected["A"]

    def reached(self, c, t):
        """(n, y, x) tap t reads from the probe of dz channel c; None outside the image"""
        n, y, x = self.probe_of[c]
        y, x = y + self.taps[t][0], x + self.taps[t][1]
        return (n, y, x) if 0 <= y < self.H and 0 <= x < self.W else None

    def probe_expected(self):
        """the probe generator's expectation read straight off the source, one element per (probe, tap, channel)"""
        xb = bf16_rne(self.src)
        E = torch.zeros(self.mblocks, self.ntaps, self.M, self.kc, dtype=torch.float64)
        for c in range(self.mblocks * self.M):
            for t in range(self.ntaps):
                p = self.reached(c, t)
                if p is not None:
                    n, y, x = p
                    E[c // self.M, t, c % self.M] = xb[n, y >> self.up0, x >> self.up0, self.coff[t]:self.coff[t] + self.kc] + 0.0
        return E

    def explain(self, mb, t, m, k, got):
        """probe: which pixel a wrong element was read from, as far as the value tells"""
        c, ch = mb * self.M + m, self.coff[t] + k
        want = self.reached(c, t)
        if ch >= self.edge_lo:
            return "probe %s tap %s channel %d (storage edges): got %r, reaches %s" % (self.probe_of[c], self.taps[t], ch, got, want)
        return "probe %s tap %s channel %d reaches %s; got %r = the source's %s %r" % (
            self.probe_of[c], self.taps[t], ch, want, got, ("y", "x", "n")[ch % 3], got - 1)

    # ---- host queries -------------------------------------------------------------------------------------------------------------
    def variant(self):
        """ssdn_wgrad_variant -> (instance in the chip-wide launch or -1, out9 = (thin, MT, CPW, NL, BOTH, PS, KS, RWX, RWD))"""
        _, lib = _lib()
        out = (C.c_int32 * 9)()
        inst = lib.ssdn_wgrad_variant(C.byref(self.a), out)
        assert inst >= -1, lib.ssdn_last_error()
        return inst, tuple(out)

    def lds_bytes(self):
        _, lib = _lib()
        return lib.ssdn_wgrad_lds_bytes(C.byref(self.a))

    def plan_key(self):
        return (self.variant()[1], self.csplit > 1, self.mblocks > 1, self.up0, self.ntiles > self.nslabs, self.tile[2] > 0)

    # ---- the device ---------------------------------------------------------------------------------------------------------------
    def poison(self):
        for t in (self.slab, self.bslab, self.gw, self.gb):
            t.fill_(float("nan"))

    def launch(self):
        """the launch alone, from poisoned slabs -> (slab, bslab) on the host, read before any reduction"""
        from ssdn.hip.engine import OpList, current_stream
        self.poison()
        OpList([("wgrad", self.a)]).run(current_stream())
        torch.cuda.synchronize()
        return self.slabs()

    def slabs(self):
        return self.slab.cpu(), self.bslab.cpu()

    def real(self, slab, bslab):
        """the real region of every slab: ([mblocks][nslabs][ntaps][M][kc], [mblocks][nslabs][M])"""
        s = slab.view(self.mblocks, self.nslabs, self.ntaps, self.Mpad, self.Kpad)[..., :self.M, :self.kc]
        return s.contiguous(), bslab.view(self.mblocks, self.nslabs, self.Mpad)[..., :self.M].contiguous()

    def check_slabs(self, slab, bslab):
        """the sum over the slabs, taken in float64 on the host, on the real region -> "max err / bound" of the rand generator (else 0)"""
        s, b = self.real(slab, bslab)
        E, Eb, A = self.expected()
        nan = int(torch.isnan(s).sum()) + int(torch.isnan(b).sum())
        assert nan == 0 and bool(torch.isfinite(s).all()) and bool(torch.isfinite(b).all()), "%d real slab elements are NaN: never stored" % nan
        S, Sb = s.double().sum(1), b.double().sum(1)
        if self.gen == "rand":
            scale = (self.N * self.H * self.W + self.nslabs) * 2.0 ** -23
            tol, tolb = scale * A, scale * self.dz.double().abs().sum((0, 1, 2)).reshape(self.mblocks, self.M)
            err, errb = (S - E).abs(), (Sb - Eb).abs()
            assert bool((err <= tol).all()) and bool((errb <= tolb).all()), "%d weight and %d bias sums beyond the bound, max err %.3e" % (
                int((err > tol).sum()), int((errb > tolb).sum()), float(err.max()))
            return max(float((err / tol.clamp_min(1e-300)).max()), float((errb / tolb.clamp_min(1e-300)).max()))
        self._same(S, E, "slab sum")
        self._same(Sb[:, None, :, None], Eb[:, None, :, None], "bias slab sum", decode=False)
        return 0.0

    def _same(self, got, want, what, decode=True):
        """bit equality of two [mblocks][ntaps][M][kc] tensors (the expectation holds no -0: the accumulators start at +0)"""
        diff = got.contiguous().view(torch.int64) != want.contiguous().view(torch.int64) if got.dtype == torch.float64 else \
            got.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)
        if bool(diff.any()):
            mb, t, m, k = (int(v) for v in diff.nonzero()[0])
            msg = "%s: %d of %d elements differ; first [block %d][tap %d][m %d][k %d]: got %r, want %r" % (
                what, int(diff.sum()), diff.numel(), mb, t, m, k, float(got[mb, t, m, k]), float(want[mb, t, m, k]))
            if self.gen == "probe" and decode:
                msg += "\n" + self.explain(mb, t, m, k, float(got[mb, t, m, k]))
            raise AssertionError(msg)

    def reduce(self):
        """SSDN_OP_WREDUCE with inv_scale = 1.0 of the slabs as they are into the poisoned gw / gb -> (gw, gb) on the host"""
        from ssdn.hip.engine import OpList, current_stream
        self.gw.fill_(float("nan"))
        self.gb.fill_(float("nan"))
        OpList([("wreduce", r) for r in self.reds]).run(current_stream())
        torch.cuda.synchronize()
        return self.gw.cpu(), self.gb.cpu()

    def check_reduced(self, gw, gb):
        """the block holds the expected values (OIHW; tap blocks: [m][c_off + t Kpad + k]), every other element is still NaN"""
        E, Eb, A = self.expected()
        M, mbs = self.M, self.mblocks
        rows = slice(M_OFF, M_OFF + mbs * M)
        if self.tapblock:
            g = gw.view(self.Mfull, self.cin_full)
            cols = slice(C_OFF, C_OFF + self.ntaps * self.Kpad)
            blk = g[rows, cols].reshape(mbs, M, self.ntaps, self.Kpad).permute(0, 2, 1, 3)
            assert self.kc == self.Kpad
        else:
            g = gw.view(self.Mfull, self.cin_full, self.ntaps)
            cols = slice(C_OFF, C_OFF + self.kc)
            blk = g[rows, cols].reshape(mbs, M, self.kc, self.ntaps).permute(0, 3, 1, 2)
        bias = gb[rows].reshape(mbs, M)
        outside = torch.ones_like(g, dtype=torch.bool)
        outside[rows, cols] = False
        assert bool(torch.isnan(g[outside]).all()), "SSDN_OP_WREDUCE wrote %d elements outside its block" % int((~torch.isnan(g[outside])).sum())
        assert bool(torch.isnan(gb[:M_OFF]).all()) and bool(torch.isnan(gb[M_OFF + mbs * M:]).all())
        assert bool(torch.isfinite(blk).all()) and bool(torch.isfinite(bias).all())
        if self.gen == "rand":
            scale = (self.N * self.H * self.W + self.nslabs) * 2.0 ** -23
            assert bool(((blk.double() - E).abs() <= scale * A).all())
            assert bool(((bias.double() - Eb).abs() <= scale * self.dz.double().abs().sum((0, 1, 2)).reshape(mbs, M)).all())
            return
        self._same(blk.contiguous(), E.float(), "reduced weight gradient")
        self._same(bias[:, None, :, None].contiguous(), Eb.float()[:, None, :, None], "reduced bias gradient", decode=False)

    def inputs_intact(self):
        """every element of the wide input tensors outside their channel windows, the guard strips included, is still NaN"""
        for d, guard, n, cs, c in self.wides:
            h = d.cpu().float()
            body = h[guard:guard + n].view(-1, cs)
            if not (bool(torch.isnan(h[:guard]).all()) and bool(torch.isnan(h[guard + n:]).all()) and bool(torch.isnan(body[:, :8]).all())
                    and bool(torch.isnan(body[:, 8 + c:]).all()) and not bool(torch.isnan(body[:, 8:8 + c]).any())):
                return False
        return True

    def check_all(self):
        """the checks of one launch alone -> the rand generator's max err / bound"""
        slab, bslab = self.launch()
        ratio = self.check_slabs(slab, bslab)
        self.check_reduced(*self.reduce())
        assert self.inputs_intact()
        return ratio


MUTANTS = {"drop": ("ints",), "seam": ("ints", "probe"), "swap_dydx": ("probe",), "trunc": ("round",), "halo": ("probe",), "swap_channels": ("ints",)}


def _row(taps, Ktot, M, NHW, tile, nslabs, want, blocks=1, src1=False, sync=False, **kw):
    return dict(taps=taps, blocks=blocks, Ktot=Ktot, M=M, NHW=NHW, tile=tile, nslabs=nslabs, want=want, src1=src1, sync=sync, kw=kw)


S8, S16, S4B, GEN = (192, 8), (64, 16), (832, 4), (0, 0)
# name -> the launch and the kernel variant it is there for: want = (MT, CPW, NL, BOTH, PS, KS) of ssdn_wgrad_variant's out9, or
# ("thin", MT).  tile = (TW, TH, TN) in pixels.  The rows behind the blank line are the classes the BASELINE plans reach beyond those
# (tests/test_wgrad_case_cpu.py::test_every_class_of_the_plans_has_a_row).
TABLE = {
    "st8": _row("B", 96, 96, (1, 32, 32), (16, 8, 1), 3, (3, 7, 4, 0) + S8),
    "st8_g2": _row("B", 96, 96, (1, 32, 32), (16, 8, 1), 3, (3, 4, 4, 0) + S8, csplit=2),
    "st8_nl2": _row("P", 48, 96, (1, 32, 32), (16, 8, 1), 3, (3, 5, 2, 0) + S8),
    "st8_nl2_m48": _row("P", 48, 48, (1, 32, 32), (16, 8, 1), 3, (2, 5, 2, 0) + S8),
    "st8_up": _row("B", 96, 96, (1, 32, 32), (16, 8, 1), 3, (3, 7, 4, 0) + S8, up0=True),
    "st16": _row("P", 32, 64, (2, 32, 32), (16, 16, 1), 3, (2, 3, 4, 0) + S16),
    "st16_k16": _row("B", 16, 96, (2, 32, 32), (16, 16, 1), 3, (3, 3, 4, 0) + S16),
    "st4b": _row("1x1", 384, 96, (1, 32, 32), (8, 8, 1), 5, (3, 4, 6, 1) + S4B, blocks=4),
    "st4b_mb4": _row("1x1", 384, 96, (1, 32, 32), (8, 8, 1), 5, (3, 4, 6, 1) + S4B, blocks=4, mblocks=4),
    "both_generic": _row("1x1", 192, 96, (1, 32, 32), (16, 4, 1), 5, (3, 2, 6, 1) + GEN, blocks=2),
    "both_single": _row("1x1", 384, 96, (1, 16, 16), (8, 8, 1), 4, (3, 4, 6, 1) + GEN, blocks=4),
    "ragged": _row("B", 96, 96, (3, 24, 40), (16, 8, 1), 4, (3, 7, 4, 0) + S8),
    "single": _row("B", 96, 96, (2, 16, 16), (16, 8, 1), 4, (3, 7, 4, 0) + GEN),
    "empty": _row("B", 96, 96, (2, 16, 16), (16, 8, 1), 6, (3, 7, 4, 0) + GEN),
    "g3_partial": _row("B", 96, 96, (2, 16, 16), (16, 8, 1), 2, (3, 3, 4, 0) + S8, csplit=3),
    "g7": _row("B", 96, 96, (2, 16, 16), (16, 8, 1), 2, (3, 1, 4, 0) + GEN, csplit=7),
    "sync": _row("P", 32, 32, (1, 16, 16), (8, 4, 1), 3, (1, 3, 4, 0) + GEN, sync=True),
    "tn8": _row("B", 96, 96, (8, 2, 2), (2, 2, 8), 1, (3, 7, 4, 0) + GEN),
    "tn16_1x2": _row("P", 96, 96, (16, 1, 2), (2, 1, 16), 1, (3, 7, 4, 0) + GEN),
    "tn2_ragged": _row("B", 96, 96, (5, 8, 8), (8, 8, 2), 2, (3, 7, 6, 1) + GEN),
    "m40_k56": _row("P", 56, 40, (2, 16, 16), (16, 8, 1), 2, (2, 5, 2, 0) + S8),
    "m88_k72": _row("P", 72, 88, (2, 16, 16), (16, 8, 1), 2, (3, 7, 4, 0) + S8),
    "m8_k8": _row("1x1", 8, 8, (2, 16, 16), (16, 8, 1), 2, (1, 1, 4, 0) + GEN),
    "head16": _row("1x1", 96, 16, (2, 16, 16), (16, 16, 1), 1, (1, 1, 4, 0) + GEN),
    "thin_k1": _row("B", 16, 32, (3, 16, 48), (16, 16, 1), 2, ("thin", 1), kreal=1),
    "thin_k2": _row("P", 16, 48, (3, 16, 48), (16, 16, 1), 2, ("thin", 2), kreal=2),
    "thin_k3": _row("B", 16, 96, (3, 16, 48), (16, 16, 1), 2, ("thin", 3), kreal=3),
    "thin_src1": _row("P", 32, 96, (1, 32, 32), (16, 16, 1), 3, ("thin", 3), src1=True, kreal=3),
    "thin_empty": _row("B", 16, 96, (1, 16, 16), (16, 16, 1), 2, ("thin", 3), kreal=3),

    "one_tap_m96": _row("1x1", 96, 96, (2, 16, 16), (16, 8, 1), 2, (3, 1, 4, 0) + GEN),                    # the 1x1 layers of the plain network
    "tn16_sync_m48": _row("B", 48, 48, (20, 2, 2), (2, 2, 16), 1, (2, 5, 4, 0) + GEN, sync=True),          # 2x2 images, 16 to a tile, the last tile ragged
    "tn4_sync_k48": _row("P", 48, 96, (6, 4, 4), (4, 4, 4), 1, (3, 5, 4, 0) + GEN, sync=True),
    "tn4_sync_k48_up": _row("B", 48, 96, (6, 4, 4), (4, 4, 4), 1, (3, 5, 4, 0) + GEN, sync=True, up0=True),
    "tn4_sync_g2": _row("B", 96, 96, (6, 4, 4), (4, 4, 4), 1, (3, 4, 4, 0) + GEN, sync=True, csplit=2),
    "tn2_both_m48": _row("B", 48, 48, (5, 8, 8), (8, 8, 2), 2, (2, 5, 6, 1) + GEN),
    "tn2_both_k48": _row("P", 48, 96, (5, 8, 8), (8, 8, 2), 2, (3, 5, 6, 1) + GEN),
    "tn2_both_k48_up": _row("B", 48, 96, (5, 8, 8), (8, 8, 2), 1, (3, 5, 6, 1) + GEN, up0=True),
    "tn2_both_g2": _row("B", 96, 96, (5, 8, 8), (8, 8, 2), 2, (3, 4, 6, 1) + GEN, csplit=2),
    "tn2_both_g2_up": _row("P", 96, 96, (5, 8, 8), (8, 8, 2), 2, (3, 4, 6, 1) + GEN, csplit=2, up0=True),
}
NAMES = list(TABLE)


_REFERENCES = {}


def make(name, gen, device=True):
    """the WCase of a row of the table; its reference is computed once per (row, generator) and shared (the operands are a function of
    the two)"""
    case = _make(name, gen, device)
    case._expected = _REFERENCES.setdefault((name, gen), {})
    return case


def _make(name, gen, device):
    r = TABLE[name]
    taps, coff = taps_of(r["taps"], r["blocks"])
    N, H, W = r["NHW"]
    c0, c1 = (0, r["Ktot"]) if r["src1"] else (r["Ktot"], 0)
    return WCase(taps, coff, c0, c1, r["kw"].get("up0", False), N, H, W, r["M"], tuple(int(v).bit_length() - 1 for v in r["tile"]), r["nslabs"],
                 csplit=r["kw"].get("csplit", 0), mblocks=r["kw"].get("mblocks", 1), kreal=r["kw"].get("kreal", 0), gen=gen,
                 seed=NAMES.index(name), device=device)


def want_out9(name):
    """the first six entries of out9 (thin rows: (1, MT)) the row is there for"""
    w = TABLE[name]["want"]
    return (1, w[1]) if w[0] == "thin" else (0,) + tuple(w)
