"""Helper (no tests): one hand-made SSDN_OP_CONV launch on tensors of its own, and its float64 reference.

Case builds the launch in channel windows of wider NaN-poisoned tensors and ref64() evaluates the formula of include/ssdn_hip.h in float64
on the same 16-bit operands.  Two operand generators: the random one (compared within check_ref's bounds, the bounds of
tests/test_hip_ops.py::test_every_op_teacher_forced), and ints=True -- small integers whose every product and partial sum is exact in
fp32 in any order, so that the expected output is an integer that does not depend on the accumulation order and the comparison is bit
equality (check_ints).  device=False builds the operands and the argument struct without a GPU (the pointers are placeholders): the
host-side queries of the library and the reference need no more.

Used by tests/test_hip_conv16.py (k_conv16 against k_conv), tests/test_hip_cdma_walk.py / tests/test_cdma_walk_cpu.py (k_cdma's tile
walk) and tests/test_hip_conv_route.py (one launch per kernel of SSDN_OP_CONV; the 1x1 layers are its only tap sets of another length)."""
import ctypes as C

import torch

SLOPE = 0.1
INT_NNZ = 32        # +-1 entries per weight row of the integer operands (see Case._int_operands for the bound this gives)
INT_IN, INT_BIAS, INT_ADD = 2, 4, 8      # |input|, |bias|, |addend| of the integer operands
INT_LIMIT = 256     # integers up to here are exact in bf16 (8 significant bits) and in fp16 (11)


def _dev():
    return torch.device("cuda:0")


def _lib():
    from ssdn.hip import lib as L
    return L, L.load()


def _rand(gen, shape, scale=1.0):
    return (torch.rand(shape, generator=gen) * 2 - 1) * scale


def _randint(gen, shape, lim):
    return torch.randint(-lim, lim + 1, shape, generator=gen).float()


def pack_signs(y):
    from interp import _pack_signs
    return _pack_signs(y)


def unrot(y, B, fill):
    """SSDN_OP_UNROT_FWD of include/ssdn_hip.h on y [4B,P,P,C] -> [B,P,P,4C]; the row the one-row shift brings in holds `fill`"""
    from interp import Interp
    s = torch.cat([torch.full_like(y[:, :1], fill), y[:, :-1]], 1)
    return torch.cat([Interp._rot(s[r * B:(r + 1) * B], a) for r, a in enumerate((0, 270, 180, 90))], -1)


def unrot_back(u, C_):
    """the rows y <= P-2 of the tensor [4B,P,P,C] whose un-rotation u [B,P,P,4C] is -> [4B,P-1,P,C]"""
    from interp import Interp
    return torch.cat([Interp._rot(u[..., r * C_:(r + 1) * C_], a)[:, 1:] for r, a in enumerate((0, 90, 180, 270))], 0)


class Case:
    """One SSDN_OP_CONV launch on tensors of its own.  Every tensor is a channel window (co = 8) of a wider one (cs = channels + 16), so a
    stride or offset taken from the wrong view shows.  (The two masks that are read as sign bytes are whole tensors: the library takes sign
    bytes only for those.)"""

    def __init__(self, role, N, c0, c1, up0, M, taps, H=16, W=16, mask=False, add=False, upsum_c=0, bias=None, seed=0, dst32=False,
                 edge=False, cm=False, ints=False, sign_out=False, mask_sign=False, upsum_mask_sign=False, urot=False, urot_smask=False,
                 kreal=0, device=True):
        from ssdn.hip.graph import choose_conv_tile
        L, lib = _lib()
        self.role, self.N, self.H, self.W, self.c0, self.c1, self.up0, self.M, self.upsum_c = role, N, H, W, c0, c1, up0, M, upsum_c
        self.ints, self.device, self.urot = ints, device, urot
        bf = role == "dgrad"
        self.dt = torch.bfloat16 if bf else torch.float16
        self.taps = [(-dy, -dx) for dy, dx in taps] if bf else list(taps)      # the data gradient walks the mirrored window
        self.Ktot, self.Mpad = c0 + c1, (M + 31) // 32 * 32
        gen = torch.Generator().manual_seed(1000 + seed)
        hs, ws = (H // 2, W // 2) if up0 else (H, W)
        self.keep = []
        self.wides = []           # every wide tensor that holds a channel window: its other channels must stay NaN

        def view(t, window=True):
            """[..., C] -> the device tensor [..., C + 16] that holds it at channel 8, and its ssdn_view"""
            if not window:
                if not device:
                    return None, L.View(0x1000, t.shape[-1], 0)
                d = t.to(_dev())
                self.keep.append(d)
                return d, L.View(d.data_ptr(), d.shape[-1], 0)
            if not device:
                return None, L.View(0x1000, t.shape[-1] + 16, 8)
            wide = torch.full(t.shape[:-1] + (t.shape[-1] + 16,), float("nan"), dtype=t.dtype)
            wide[..., 8:8 + t.shape[-1]] = t
            d = wide.to(_dev())
            self.keep.append(d)
            self.wides.append((d, t.shape[-1]))
            return d, L.View(d.data_ptr(), d.shape[-1], 8)

        def raw(t):
            """a plain device buffer -> its address"""
            if not device:
                return 0x1000
            d = t.to(_dev())
            self.keep.append(d)
            return d.data_ptr()

        if ints:
            s0, s1, w, bias_t, mask_t, add_t, umask_t = self._int_operands(gen, bias, mask, add, hs, ws)
        else:
            s0 = _rand(gen, (N, hs, ws, c0)) if c0 else None
            s1 = _rand(gen, (N, H, W, c1)) if c1 else None
        if kreal:                 # a first layer: kreal real input channels, the slots behind them hold zeros (ssdn_conv_args.kreal)
            s0[..., kreal:] = 0
        if edge:
            # non-zero only where the halo's zero fill begins: the two rows next to the rows above (forward) / below (data gradient) the
            # image, and the left and right columns
            for s in (s0, s1):
                if s is None:
                    continue
                keep = torch.zeros_like(s)
                rows = slice(s.shape[1] - 2, None) if bf else slice(0, 2)
                keep[:, rows] = s[:, rows]
                keep[:, :, 0] = s[:, :, 0]
                keep[:, :, -1] = s[:, :, -1]
                s.copy_(keep)
        self.s0 = s0.to(self.dt) if c0 else None
        self.s1 = s1.to(self.dt) if c1 else None
        if ints:
            self.w, self.bias, self.mask, self.add, self.umask = w.to(self.dt), bias_t, mask_t, add_t, umask_t
        else:
            w = _rand(gen, (len(self.taps), self.Mpad, self.Ktot), 1.0 / (3.0 * self.Ktot ** 0.5))
            w[:, M:] = 0
            self.w = w.to(self.dt)
            self.bias = _rand(gen, (M,), 0.3) if (bias if bias is not None else not bf) else None
            self.mask = _rand(gen, (N, H, W, M)).to(torch.float16) if mask else None
            self.add = _rand(gen, (N, H, W, M)).to(self.dt) if add else None
            self.umask = _rand(gen, (N, H // 2, W // 2, upsum_c)).to(torch.float16) if upsum_c else None
        self.dw = self.w.to(_dev()) if device else None
        self.dbias = self.bias.to(_dev()) if self.bias is not None and device else None

        a = L.ConvArgs()
        if c0:
            _, a.src0 = view(self.s0)
        if c1:
            _, a.src1 = view(self.s1)
        a.c0, a.c1, a.up0, a.N, a.H, a.W, a.ntaps = c0, c1, int(up0), N, H, W, len(self.taps)
        for t, (dy, dx) in enumerate(self.taps):
            a.dy[t], a.dx[t] = dy, dx
        a.w, a.M, a.Mpad, a.Ktot = (self.dw.data_ptr() if device else 0x1000), M, self.Mpad, self.Ktot
        if self.bias is not None:
            a.bias = self.dbias.data_ptr() if device else 0x1000
        a.act = int(not bf and not ints)          # (the integer operands: no LeakyReLU)
        if mask:
            _, a.mask = view(self.mask, window=not mask_sign)
            if mask_sign:
                a.mask_sign = raw(pack_signs(self.mask.float()))
        if add:
            _, a.add = view(self.add)
        self.outs = {}
        self.bytes_out = {}       # sign-byte outputs: poisoned with 0xA5
        if dst32 and not device:
            a.dst32 = 0x1000
        elif dst32:
            self.outs["dst32"] = torch.empty(N, M, H, W, device=_dev())
            a.dst32 = self.outs["dst32"].data_ptr()
        elif urot:
            self.outs["urot"], a.urot = view(torch.zeros(N // 4, H, W, 4 * M, dtype=self.dt))
            if urot_smask:
                a.urot_smask = self._bytes("urot_smask", (N, H, W, M // 8))
        else:
            self.outs["dst"], a.dst = view(torch.zeros(N, H, W, M, dtype=self.dt))
        if sign_out:
            a.sign_out = self._bytes("sign_out", (N, H, W, M // 8))
        if upsum_c:
            self.outs["upsum"], a.upsum = view(torch.zeros(N, H // 2, W // 2, upsum_c, dtype=self.dt))
            _, a.upsum_mask = view(self.umask, window=not upsum_mask_sign)
            if upsum_mask_sign:
                a.upsum_mask_sign = raw(pack_signs(self.umask.float()))
            a.upsum_c = upsum_c
        cus = lib.ssdn_device_cus()
        a.ltw, a.lth, a.ltn, a.kc = choose_conv_tile(N, H, W, self.taps, self.Ktot, self.Mpad, out16=not dst32, cus=cus if cus > 0 else 256)
        a.bf16, a.kreal = int(bf), kreal or self.Ktot
        if cm:
            # the chunk-major copy SSDN_OP_WPACK writes next to the shadow (ssdn_conv_args.wc), by the host model tests/test_hip_optimiser.py
            # holds that op to: chunks of 48 input channels, then one optional chunk of 16
            from optim_ref import chunk_major_positions
            pos = torch.from_numpy(chunk_major_positions(9, self.Mpad, self.Ktot).reshape(-1).copy())
            wc = torch.zeros(9 * self.Mpad * self.Ktot, dtype=torch.int16)
            wc[pos] = self.w.view(torch.int16).reshape(-1)
            self.wc = wc
            self.dwc = wc.to(_dev()) if device else None
            a.wc = self.dwc.data_ptr() if device else 0x1000
        self.a = a

    def _bytes(self, name, shape):
        if not self.device:
            return 0x1000
        self.bytes_out[name] = torch.full(shape, 0xA5, dtype=torch.uint8, device=_dev())
        return self.bytes_out[name].data_ptr()

    def _int_operands(self, gen, bias, mask, add, hs, ws):
        """Integer operands.  Inputs dense in {-2..2}; each output channel's weight row has INT_NNZ entries +-1 at hashed (tap, channel)
        positions -- row m takes positions m INT_NNZ .. (m + 1) INT_NNZ - 1 (mod 9 Ktot) of one hashed permutation of all positions, so
        the rows differ and every position is hit by floor or ceil(M INT_NNZ / 9 Ktot) rows; bias in {-4..4}, addend in {-8..8}; the masks
        are positive (factor exactly 1: the launch keeps its mask operand and so its kernel instantiation).  Worst case
        |v| <= 2 INT_NNZ + 4 + 8 = 76 and a fused 2x2 up-sum (no bias, mask or addend there) <= 4 * 2 INT_NNZ = 256 = INT_LIMIT."""
        N, H, W, M, Ktot = self.N, self.H, self.W, self.M, self.Ktot
        bf = self.role == "dgrad"
        s0 = _randint(gen, (N, hs, ws, self.c0), INT_IN) if self.c0 else None
        s1 = _randint(gen, (N, H, W, self.c1), INT_IN) if self.c1 else None
        P = 9 * Ktot
        assert INT_NNZ <= P
        perm = torch.randperm(P, generator=gen)
        pos = perm[(torch.arange(M)[:, None] * INT_NNZ + torch.arange(INT_NNZ)[None, :]) % P]        # [M][INT_NNZ] -> tap * Ktot + k
        sign = torch.randint(0, 2, (M, INT_NNZ), generator=gen).float() * 2 - 1
        w = torch.zeros(9, self.Mpad, Ktot)
        w[pos // Ktot, torch.arange(M)[:, None].expand_as(pos), pos % Ktot] = sign
        self.w_hits = torch.bincount(pos.reshape(-1), minlength=P)                                  # rows per (tap, channel) position
        bias_t = _randint(gen, (M,), INT_BIAS) if (bias if bias is not None else not bf) else None
        mask_t = (torch.rand((N, H, W, M), generator=gen) + 0.5).to(torch.float16) if mask else None
        add_t = _randint(gen, (N, H, W, M), INT_ADD).to(self.dt) if add else None
        umask_t = (torch.rand((N, H // 2, W // 2, self.upsum_c), generator=gen) + 0.5).to(torch.float16) if self.upsum_c else None
        return s0, s1, w, bias_t, mask_t, add_t, umask_t

    def eligible(self):
        L, lib = _lib()
        return lib.ssdn_conv16_eligible(C.byref(self.a))

    def split(self):
        """ssdn_conv_dma_split -> (k_cdma serves the launch, {tiles_x, tiles_y, segs, tps, nitems, grid, xcd_map, mt_blocks})"""
        L, lib = _lib()
        out = (C.c_int32 * 8)()
        rc = lib.ssdn_conv_dma_split(C.byref(self.a), out)
        assert rc >= 0, lib.ssdn_last_error()
        return rc, dict(zip(("tiles_x", "tiles_y", "segs", "tps", "nitems", "grid", "xcd_map", "mt_blocks"), out))

    def launch(self):
        """the launch from poisoned outputs -> {name: the whole (wide) output tensor}, on the host"""
        from ssdn.hip.engine import OpList, current_stream
        for t in self.outs.values():
            t.fill_(float("nan"))
        for t in self.bytes_out.values():
            t.fill_(0xA5)
        OpList([("conv", self.a)]).run(current_stream())
        torch.cuda.synchronize()
        got = {k: t.detach().cpu().clone() for k, t in self.outs.items()}
        got.update({k: t.detach().cpu().clone() for k, t in self.bytes_out.items()})
        return got

    def run(self, roles):
        """the launch with k_conv16 allowed for `roles`, from poisoned outputs -> {name: bits of the whole (wide) output tensor}"""
        L, lib = _lib()
        L.check(lib.ssdn_conv_set_conv16(roles))
        return self.launch()

    def inputs_intact(self):
        """the channels of the wide input tensors outside their windows are still NaN (outputs: check_ref / check_ints look at theirs)"""
        outs = {id(t) for t in self.outs.values()}
        return all(bool(torch.isnan(d[..., :8].float()).all()) and bool(torch.isnan(d[..., 8 + c:].float()).all())
                   for d, c in self.wides if id(d) not in outs)

    def ref64(self, dev=None):
        """float64 convolution of the 16-bit operands by the formula of include/ssdn_hip.h -> (dst [N,H,W,M], upsum or None); dev: where
        to evaluate it (default: the host)"""
        N, H, W = self.N, self.H, self.W
        to = (lambda t: t.to(dev)) if dev is not None else (lambda t: t)
        parts = []
        if self.c0:
            s = to(self.s0).double()
            if self.up0:
                s = s.repeat_interleave(2, 1).repeat_interleave(2, 2)
            parts.append(s)
        if self.c1:
            parts.append(to(self.s1).double())
        x = torch.cat(parts, -1)
        xp = torch.zeros(N, H + 4, W + 4, self.Ktot, dtype=torch.float64, device=x.device)
        xp[:, 2:2 + H, 2:2 + W] = x
        w = to(self.w).double()
        v = torch.zeros(N, H, W, self.M, dtype=torch.float64, device=x.device)
        for t, (dy, dx) in enumerate(self.taps):
            v += torch.einsum("nyxk,mk->nyxm", xp[:, 2 + dy:2 + dy + H, 2 + dx:2 + dx + W], w[t, :self.M])
        if self.bias is not None:
            v += to(self.bias).double()
        if self.a.act:
            v = torch.where(v > 0, v, SLOPE * v)
        conv = v.clone()
        if self.add is not None:
            v = v + to(self.add).double()
        if self.mask is not None:
            v = v * torch.where(to(self.mask).double() > 0, 1.0, SLOPE)
        up = None
        if self.upsum_c:
            u = v[..., :self.upsum_c]
            g = torch.where(to(self.umask).double() > 0, 1.0, SLOPE)
            up = (u[:, 0::2, 0::2] + u[:, 0::2, 1::2] + u[:, 1::2, 0::2] + u[:, 1::2, 1::2]) * g
            self.up_abs = (u[:, 0::2, 0::2].abs() + u[:, 0::2, 1::2].abs() + u[:, 1::2, 0::2].abs() + u[:, 1::2, 1::2].abs()) * g
        return v, up, conv

    def ints_expected(self, dev=None):
        """the integer operands' expected outputs {name: the whole wide tensor, NaN where the launch stores nothing}, after asserting the
        condition that makes them exact in any accumulation order and in the 16-bit output type: every value, fused 2x2 up-sums included,
        is an integer of magnitude <= INT_LIMIT"""
        assert self.ints
        ref, up, _ = self.ref64(dev)
        for r in (ref, up):
            if r is not None:
                assert bool((r == r.round()).all()) and float(r.abs().max()) <= INT_LIMIT, "integer reference: |v| max %g" % float(r.abs().max())
        M, uc = self.M, self.upsum_c
        ref, up = ref + 0.0, (up + 0.0 if up is not None else None)       # (a zero is +0: the accumulators start at +0)

        def wide(t, lo=0):
            o = torch.full(t.shape[:-1] + (t.shape[-1] + 16,), float("nan"), dtype=self.dt, device=t.device)
            o[..., 8 + lo:8 + t.shape[-1]] = t[..., lo:].to(self.dt)
            return o
        if self.urot:
            return {"urot": wide(unrot(ref, self.N // 4, float("nan")))}
        out = {"dst": wide(ref, uc)}
        if uc:
            out["upsum"] = wide(up)
        return out


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(new, old, what):
    assert new.keys() == old.keys()
    for k in new:
        diff = _bits(new[k]) != _bits(old[k])
        assert not bool(diff.any()), "%s: %s differs in %d of %d elements" % (what, k, int(diff.sum()), diff.numel())


def _check_ref(case, got, sparse=False, dev=None):
    """the bounds of test_every_op_teacher_forced: one ulp of the storage type (fp16 2e-3, bf16 1.6e-2) of the element + 1e-2 of that of the
    largest; with an addend one more rounding relative to the addends; the fused up-sum 1.6e-2 of the element + 2e-2 of the mean.
    sparse (the border-values-only inputs, where most up-sums are exactly zero and the mean says nothing about an element's addends): the
    up-sum's bound is what that mean stands for, written out -- each of the four bf16 addends within one bf16 ulp (2^-8) of ITS size, plus
    one ulp of the sum for its own rounding.
    dev: evaluate the reference and the comparison there (the large cases); a fused UNROT_FWD output (case.urot) is compared in its
    un-rotated place, and the rows the shift leaves empty must still be NaN."""
    ref, up, conv = case.ref64(dev)
    if dev is not None:
        got = {k: v.to(dev) for k, v in got.items()}
    M, uc = case.M, case.upsum_c
    ulp = 1.6e-2 if case.role == "dgrad" else 2e-3
    tol = ulp * ref.abs() + ulp * float(ref.abs().max()) * 1e-2 + 1e-9
    if case.add is not None:
        add, mask = (case.add.to(ref.device), case.mask.to(ref.device) if case.mask is not None else None)
        scale = torch.where(mask.double() > 0, 1.0, SLOPE) if mask is not None else 1.0
        tol = tol + ulp * (add.double().abs() + conv.abs()) * scale
    key, Mw = "dst", M
    if case.urot:
        key, Mw, B = "urot", 4 * M, case.N // 4
        ref, tol = unrot(ref, B, float("nan")), unrot(tol, B, 0.0)
        empty = torch.isnan(ref)
        assert bool(torch.isnan(got[key][..., 8:8 + Mw][empty].float()).all()), "the rows the shift leaves empty were written"
        ref = torch.where(empty, 0.0, ref)
        got = dict(got)
        got[key] = got[key].clone()
        got[key][..., 8:8 + Mw][empty] = 0
    g = got[key][..., 8:8 + Mw].double()
    err = (g - ref).abs()[..., uc:]
    print("%s N %d %d+%d->%d: max err / bound %.4f" % (case.role, case.N, case.c0, case.c1, M, float((err / tol[..., uc:]).max())))
    assert bool(torch.isfinite(g[..., uc:]).all())
    assert bool((err <= tol[..., uc:]).all()), "dst: %d elements beyond the bound, max err %.3e" % (int((err > tol[..., uc:]).sum()), float(err.max()))
    # what the launch does not own stays poisoned: the guard channels, and the channels that only exist as up-sums
    assert bool(torch.isnan(got[key][..., :8].float()).all()) and bool(torch.isnan(got[key][..., 8 + Mw:].float()).all())
    if uc:
        assert bool(torch.isnan(got["dst"][..., 8:8 + uc].float()).all())
        gu = got["upsum"][..., 8:8 + uc].double()
        tolu = 1.6e-2 * up.abs() + 2e-2 * float(up.abs().mean()) + 1e-9
        if sparse:
            tolu = 2.0 ** -8 * (case.up_abs + up.abs()) + 1e-9
        erru = (gu - up).abs()
        print("  fused up-sum: max err / bound %.4f" % float((erru / tolu).max()))
        assert bool((erru <= tolu).all()), "upsum: %d elements beyond the bound" % int((erru > tolu).sum())
        assert bool(torch.isnan(got["upsum"][..., :8].float()).all()) and bool(torch.isnan(got["upsum"][..., 8 + uc:].float()).all())


def check_ints(case, got, dev=None):
    """bit equality of every 16-bit output -- the whole wide tensor: the window holds the float64 reference cast to the output type, every
    other element (guard channels, the channels that only exist as up-sums, the rows a fused UNROT_FWD leaves empty) is still the NaN it was"""
    want = case.ints_expected(dev)
    for k, w in want.items():
        g = got[k].to(w.device)
        diff = _bits(g) != _bits(w)
        nan_left = int((torch.isnan(g.float()) & ~torch.isnan(w.float())).sum())
        assert not bool(diff.any()), "%s: %d of %d elements differ from the exact integers (%d of them still NaN: never stored)" % (
            k, int(diff.sum()), diff.numel(), nan_left)


def check_signs(case, got):
    """sign bytes are exact: those of the output the launch itself stored.  sign_out: every pixel; urot_smask: the rows y <= P-2 of the
    layer's output (what the un-rotation reads), row P-1 untouched"""
    M = case.M
    if "sign_out" in got:
        own = pack_signs(got["dst"][..., 8:8 + M].float())
        assert torch.equal(got["sign_out"], own), "%d sign bytes differ from the signs of the stored output" % int((got["sign_out"] != own).sum())
    if "urot_smask" in got:
        own = pack_signs(unrot_back(got["urot"][..., 8:8 + 4 * M].float(), M))
        s = got["urot_smask"]
        assert torch.equal(s[:, :-1], own), "%d sign bytes differ from the signs of the stored output" % int((s[:, :-1] != own).sum())
        assert bool((s[:, -1] == 0xA5).all()), "sign bytes of the cut-off row were written"
