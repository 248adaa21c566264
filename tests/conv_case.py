"""Helper (no tests): one hand-made SSDN_OP_CONV launch on tensors of its own, and its float64 reference.

Case builds the launch in channel windows of wider NaN-poisoned tensors and ref64() evaluates the formula of include/ssdn_hip.h in float64
on the same 16-bit operands.  Two operand generators: the random one (compared within check_ref's bounds, the bounds of
tests/test_hip_ops.py::test_every_op_teacher_forced), and ints=True -- small integers whose every product and partial sum is exact in
fp32 in any order, so that the expected output is an integer that does not depend on the accumulation order and the comparison is bit
equality (check_ints).  device=False builds the operands and the argument struct without a GPU (the pointers are placeholders): the
host-side queries of the library and the reference need no more.

The 1x1 layers (one tap; k_gdma, csrc/gemm_dma.hip) have more: the fused SSDN_OP_UNROT_BWD (unrot=True: the output goes, un-rotated and
times LeakyReLU' of unrot_mask, to `unrot`), a second, narrow 1x1 layer behind the first (next=dict(M4, bias, act): two SSDN_OP_CONV
records in one list, fp32 NCHW output), and under ints=True the LeakyReLU and masks of both signs -- what follows the exact integer sum is
a fixed chain of fp32 operations and one round-to-nearest-even conversion, which ints_expected() repeats in torch float32.

Used by tests/test_hip_conv16.py (k_conv16 against k_conv), tests/test_hip_cdma_walk.py / tests/test_cdma_walk_cpu.py (k_cdma's tile
walk), tests/test_hip_conv_route.py (one launch per kernel of SSDN_OP_CONV) and tests/test_hip_gdma_walk.py / tests/test_gdma_walk_cpu.py
(k_gdma's tile walk and epilogues), and by tests/test_hip_conv_walk.py / tests/test_conv_walk_cpu.py (k_conv per launch), which need the
rest: tile=(ltw, lth, ltn, kc) in place of the planner's tiling; pool=True (pool_shifted 0 / 1): the fused max-pool output, a channel window
of a wide tensor of its own; act=True under ints=True on a 3x3 layer (the fused pool needs the activation) and ints=True with dst32 -- both
follow the exact integer sum with the kernel's fixed fp32 chain (ints_expected)."""
import ctypes as C

import torch

SLOPE = 0.1
INT_NNZ = 32        # +-1 entries per weight row of the integer operands (see Case._int_operands for the bound this gives)
INT_IN, INT_BIAS, INT_ADD = 2, 4, 8      # |input|, |bias|, |addend| of the integer operands
INT_LIMIT = 256     # integers up to here are exact in bf16 (8 significant bits) and in fp16 (11)
NEXT_GUARD = 256    # fp32 elements in front of and behind the second layer's output (and a dst32 output) that must stay NaN
VARIANT_FIELDS = ("MT", "BF", "KS", "threads", "path", "nblk", "tiles", "m_base")      # ssdn_conv_variant, per launch
PATHS = ("pipe", "async", "allw", "flat")                                              # ... its `path`


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


def unrot_bwd(u, C_):
    """the adjoint of unrot(): SSDN_OP_UNROT_BWD of include/ssdn_hip.h without its mask, u [B,P,P,4C] -> [4B,P,P,C]; row P-1, which the
    shift cut off, holds zeros"""
    y = unrot_back(u, C_)
    return torch.cat([y, torch.zeros_like(y[:, :1])], 1)


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
                 kreal=0, device=True, unrot=False, unrot_smask=False, next=None, tile=None, pool=False, pool_shifted=0, act=None):
        from ssdn.hip.graph import choose_conv_tile
        L, lib = _lib()
        self.role, self.N, self.H, self.W, self.c0, self.c1, self.up0, self.M, self.upsum_c = role, N, H, W, c0, c1, up0, M, upsum_c
        self.ints, self.device, self.urot, self.unrot, self.next = ints, device, urot, unrot, next
        self.pool, self.pool_shifted = pool, pool_shifted
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
        # (the operands of the 1x1 layers' extras are drawn behind everything else: the callers without them get what they always got)
        self.unrot_mask = _rand(gen, (4 * N, H, W, M // 4)).to(torch.float16) if unrot else None
        if next is not None:
            self._next_operands(gen, next)
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
        # (the integer operands: no LeakyReLU -- but for a 1x1 layer, whose expectation follows the fp32 chain behind the sum; in front of a
        # second layer the tile must hold integers)
        a.act = int(not bf and (not ints or (len(self.taps) == 1 and next is None)))
        if act is not None:       # (integer operands on a 3x3 layer with the activation: ints_expected follows the fp32 chain there too)
            assert not bf and not mask and not add
            a.act = int(act)
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
            # (NEXT_GUARD elements in front of and behind the output: launch() leaves them in dst32_guards, still NaN if nothing stored there)
            self.dst32_buf = torch.empty(N * M * H * W + 2 * NEXT_GUARD, device=_dev())
            self.outs["dst32"] = self.dst32_buf[NEXT_GUARD:NEXT_GUARD + N * M * H * W].view(N, M, H, W)
            a.dst32 = self.outs["dst32"].data_ptr()
        elif urot:
            self.outs["urot"], a.urot = view(torch.zeros(N // 4, H, W, 4 * M, dtype=self.dt))
            if urot_smask:
                a.urot_smask = self._bytes("urot_smask", (N, H, W, M // 8))
        else:
            self.outs["dst"], a.dst = view(torch.zeros(N, H, W, M, dtype=self.dt))
        if unrot:
            # the conv's N is the batch: the output channel block r of image b belongs to image r N + b of the rotated stack
            self.outs["unrot"], a.unrot = view(torch.zeros(4 * N, H, W, M // 4, dtype=self.dt))
            if unrot_smask:
                # the bytes SSDN_OP_UNROT_FWD writes (oracle/interp.py): 12 per pixel, the cut-off row P-1 untouched; the activation
                # itself must then not be read: it holds NaN, which the kernel's sign test would take for "positive"
                sb = pack_signs(self.unrot_mask.float())
                sb[:, -1] = 0xA5
                a.unrot_smask = raw(sb)
                _, a.unrot_mask = view(torch.full_like(self.unrot_mask, float("nan")))
            else:
                _, a.unrot_mask = view(self.unrot_mask)
        if sign_out:
            a.sign_out = self._bytes("sign_out", (N, H, W, M // 8))
        if pool:
            self.outs["pool"], a.pool = view(torch.zeros(N, H // 2, W // 2, M, dtype=self.dt))
            a.pool_shifted = pool_shifted
        if upsum_c:
            self.outs["upsum"], a.upsum = view(torch.zeros(N, H // 2, W // 2, upsum_c, dtype=self.dt))
            _, a.upsum_mask = view(self.umask, window=not upsum_mask_sign)
            if upsum_mask_sign:
                a.upsum_mask_sign = raw(pack_signs(self.umask.float()))
            a.upsum_c = upsum_c
        cus = lib.ssdn_device_cus()
        a.ltw, a.lth, a.ltn, a.kc = tile or choose_conv_tile(N, H, W, self.taps, self.Ktot, self.Mpad, out16=not dst32, cus=cus if cus > 0 else 256)
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
        if next is not None:
            a4 = L.ConvArgs()
            a4.src0 = L.View(a.dst.p, a.dst.cs, a.dst.co)
            a4.c0, a4.c1, a4.up0, a4.N, a4.H, a4.W, a4.ntaps = M, 0, 0, N, H, W, 1
            self.dw4 = self.w4.to(_dev()) if device else None
            self.dbias4 = self.bias4.to(_dev()) if self.bias4 is not None and device else None
            a4.w, a4.M, a4.Mpad, a4.Ktot = (self.dw4.data_ptr() if device else 0x1000), next["M4"], 32, M
            if self.bias4 is not None:
                a4.bias = self.dbias4.data_ptr() if device else 0x1000
            a4.act = int(bool(next.get("act")))
            self.next_n = N * next["M4"] * H * W
            self.next_buf = torch.empty(self.next_n + 2 * NEXT_GUARD, device=_dev()) if device else None
            a4.dst32 = self.next_buf.data_ptr() + 4 * NEXT_GUARD if device else 0x1000
            a4.ltw, a4.lth, a4.ltn, a4.kc = choose_conv_tile(N, H, W, self.taps, M, 32, out16=False, cus=cus if cus > 0 else 256)
            a4.bf16, a4.kreal = 0, M
            self.a4 = a4

    def _next_operands(self, gen, next):
        """the second layer's weights [1][32][M] (rows >= M4: zeros) and bias.  Integer operands: INT_NNZ entries +-1 per row and a bias in
        {-4..4} on the first layer's integers (no activation there: |.| <= 2 INT_NNZ + 4 = 68), so |out| <= 32 * 68 + 4 -- exact in fp32"""
        M4 = next["M4"]
        if self.ints:
            w4 = torch.zeros(1, 32, self.M)
            for m in range(M4):
                w4[0, m, torch.randperm(self.M, generator=gen)[:INT_NNZ]] = torch.randint(0, 2, (INT_NNZ,), generator=gen).float() * 2 - 1
            b4 = _randint(gen, (M4,), INT_BIAS)
        else:
            w4 = _rand(gen, (1, 32, self.M), 1.0 / (3.0 * self.M ** 0.5))
            w4[:, M4:] = 0
            b4 = _rand(gen, (M4,), 0.3)
        self.w4, self.bias4 = w4.to(torch.float16), (b4 if next.get("bias") else None)

    def _bytes(self, name, shape):
        if not self.device:
            return 0x1000
        self.bytes_out[name] = torch.full(shape, 0xA5, dtype=torch.uint8, device=_dev())
        return self.bytes_out[name].data_ptr()

    def _int_operands(self, gen, bias, mask, add, hs, ws):
        """Integer operands.  Inputs dense in {-2..2}; each output channel's weight row has INT_NNZ entries +-1 at hashed (tap, channel)
        positions -- row m takes positions m INT_NNZ .. (m + 1) INT_NNZ - 1 (mod ntaps Ktot) of one hashed permutation of all positions, so
        the rows differ and every position is hit by floor or ceil(M INT_NNZ / (ntaps Ktot)) rows; bias in {-4..4}, addend in {-8..8}; the masks
        are positive (factor exactly 1: the launch keeps its mask operand and so its kernel instantiation) -- but for a 1x1 layer, whose
        masks take both signs.  Worst case |v| <= 2 INT_NNZ + 4 + 8 = 76 and a fused 2x2 up-sum (no bias, mask or addend there)
        <= 4 * 2 INT_NNZ = 256 = INT_LIMIT; one tap (Ktot >= INT_NNZ, no addend): |v| <= 2 INT_NNZ + 4 = 68."""
        N, H, W, M, Ktot = self.N, self.H, self.W, self.M, self.Ktot
        bf = self.role == "dgrad"
        s0 = _randint(gen, (N, hs, ws, self.c0), INT_IN) if self.c0 else None
        s1 = _randint(gen, (N, H, W, self.c1), INT_IN) if self.c1 else None
        ntaps = len(self.taps)
        P = ntaps * Ktot
        nnz = min(INT_NNZ, P)     # (a 1x1 layer of 16 input channels has only 16 positions: every one is hit, the bounds only shrink)
        perm = torch.randperm(P, generator=gen)
        pos = perm[(torch.arange(M)[:, None] * nnz + torch.arange(nnz)[None, :]) % P]                # [M][nnz] -> tap * Ktot + k
        sign = torch.randint(0, 2, (M, nnz), generator=gen).float() * 2 - 1
        w = torch.zeros(ntaps, self.Mpad, Ktot)
        w[pos // Ktot, torch.arange(M)[:, None].expand_as(pos), pos % Ktot] = sign
        self.w_hits = torch.bincount(pos.reshape(-1), minlength=P)                                  # rows per (tap, channel) position
        bias_t = _randint(gen, (M,), INT_BIAS) if (bias if bias is not None else not bf) else None
        mask_t = (torch.rand((N, H, W, M), generator=gen) + 0.5).to(torch.float16) if mask else None
        if mask and ntaps == 1:        # a 1x1 layer: both signs (ints_expected follows the epilogue's fp32 chain)
            mask_t = ((mask_t.float() - 1.0) * 2).to(torch.float16)
        add_t = _randint(gen, (N, H, W, M), INT_ADD).to(self.dt) if add else None
        umask_t = (torch.rand((N, H // 2, W // 2, self.upsum_c), generator=gen) + 0.5).to(torch.float16) if self.upsum_c else None
        return s0, s1, w, bias_t, mask_t, add_t, umask_t

    def eligible(self):
        L, lib = _lib()
        return lib.ssdn_conv16_eligible(C.byref(self.a))

    def variant(self):
        """ssdn_conv_variant -> the k_conv launches the op makes: a list of {MT, BF, KS, threads, path, nblk, tiles, m_base} (empty: another
        kernel serves it)"""
        L, lib = _lib()
        out = (C.c_int32 * 16)()
        rc = lib.ssdn_conv_variant(C.byref(self.a), out)
        assert rc >= 0, lib.ssdn_last_error()
        return [dict(zip(VARIANT_FIELDS, out[8 * i:8 * i + 8])) for i in range(rc)]

    def split(self):
        """ssdn_conv_dma_split -> (k_cdma serves the launch, {tiles_x, tiles_y, segs, tps, nitems, grid, xcd_map, mt_blocks})"""
        L, lib = _lib()
        out = (C.c_int32 * 8)()
        rc = lib.ssdn_conv_dma_split(C.byref(self.a), out)
        assert rc >= 0, lib.ssdn_last_error()
        return rc, dict(zip(("tiles_x", "tiles_y", "segs", "tps", "nitems", "grid", "xcd_map", "mt_blocks"), out))

    def launch(self):
        """the launch (with next: the two records in one list) from poisoned outputs -> {name: the whole (wide) output tensor}, on the host"""
        from ssdn.hip.engine import OpList, current_stream
        for t in self.outs.values():
            t.fill_(float("nan"))
        for t in self.bytes_out.values():
            t.fill_(0xA5)
        if self.next is not None:
            self.next_buf.fill_(float("nan"))
        if "dst32" in self.outs:
            self.dst32_buf.fill_(float("nan"))
        OpList([("conv", self.a)] + ([("conv", self.a4)] if self.next is not None else [])).run(current_stream())
        torch.cuda.synchronize()
        got = {k: t.detach().cpu().clone() for k, t in self.outs.items()}
        if "dst32" in self.outs:
            self.dst32_guards = torch.cat([self.dst32_buf[:NEXT_GUARD], self.dst32_buf[-NEXT_GUARD:]]).cpu()
        got.update({k: t.detach().cpu().clone() for k, t in self.bytes_out.items()})
        if self.next is not None:
            got["next32"] = self.next_buf.detach().cpu().clone()       # (with its guards)
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
        self.pre = v.clone()           # the sum itself: what ints_expected's fp32 chain of a 1x1 layer starts from
        if self.a.act:
            v = torch.where(v > 0, v, SLOPE * v)
        if self.unrot:
            # fused SSDN_OP_UNROT_BWD: everything below is in the rotated stack's place [4N,P,P,M/4]
            self.pre, v = unrot_bwd(self.pre, self.M // 4), unrot_bwd(v, self.M // 4) * torch.where(to(self.unrot_mask).double() > 0, 1.0, SLOPE)
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

    def next_ref64(self, first, dev=None, act=True):
        """the second layer in float64 on `first` [N,H,W,M], the first layer's rounded 16-bit output -> [N,M4,H,W]; act=False: without
        its activation"""
        to = (lambda t: t.to(dev)) if dev is not None else (lambda t: t)
        M4 = self.next["M4"]
        v = torch.einsum("nyxk,mk->nmyx", to(first).double(), to(self.w4).double()[0, :M4])
        if self.bias4 is not None:
            v += to(self.bias4).double()[None, :, None, None]
        return torch.where(v > 0, v, SLOPE * v) if self.a4.act and act else v

    def _ints_chain(self, dev=None):
        """a 1x1 layer's integer expectation.  The sum v is an exact integer in any order; what k_gdma does behind it is a fixed chain
        of fp32 operations and round-to-nearest-even conversions, repeated here in torch float32: forward max(v, 0.1f v) -> fp16;
        data gradient bf16(v), then * (mask > 0 ? 1 : 0.1f) -> bf16 (the fused un-rotation: the same on unrot_mask, zeros in row P-1);
        a second layer: its exact integer sum + bias in fp32, v > 0 ? v : 0.1f v."""
        self.ref64(dev)
        pre = self.pre
        assert bool((pre == pre.round()).all()) and float(pre.abs().max()) <= INT_LIMIT, "integer reference: |v| max %g" % float(pre.abs().max())
        slope = torch.tensor(SLOPE, dtype=torch.float32, device=pre.device)
        one = torch.ones((), dtype=torch.float32, device=pre.device)
        x = pre.float() + 0.0
        if self.a.dst32:      # k_conv's fp32 NCHW output: the integer sum (+ bias) in fp32, then v > 0 ? v : 0.1f v; nothing else is applied
            return {"dst32": (torch.where(x > 0, x, x * slope) if self.a.act else x).permute(0, 3, 1, 2).contiguous()}
        if self.a.act:
            x = torch.maximum(x, x * slope)
        x = x.to(self.dt)
        mask = self.unrot_mask if self.unrot else self.mask
        if mask is not None:
            x = (x.float() * torch.where(mask.to(pre.device).float() > 0, one, slope)).to(self.dt)

        def wide(t):
            o = torch.full(t.shape[:-1] + (t.shape[-1] + 16,), float("nan"), dtype=self.dt, device=t.device)
            o[..., 8:8 + t.shape[-1]] = t
            return o
        if self.unrot:      # nothing goes to dst
            return {"unrot": wide(x), "dst": torch.full((self.N, self.H, self.W, self.M + 16), float("nan"), dtype=self.dt, device=x.device)}
        out = {"dst": wide(x)}
        if self.next is not None:
            y = self.next_ref64(x, dev, act=False)
            assert bool((y == y.round()).all()) and float(y.abs().max()) <= INT_NNZ * (2 * INT_NNZ + INT_BIAS) + INT_BIAS
            y = y.float() + 0.0
            if self.a4.act:
                y = torch.where(y > 0, y, y * slope)
            buf = torch.full((self.next_n + 2 * NEXT_GUARD,), float("nan"), dtype=torch.float32, device=y.device)
            buf[NEXT_GUARD:NEXT_GUARD + self.next_n] = y.reshape(-1)
            out["next32"] = buf
        return out

    def _ints_act(self, dev=None):
        """a 3x3 layer's integer expectation with the activation and / or the fp32 output.  The sum (+ bias) v is an exact integer in any
        order; k_conv follows it with v > 0 ? v : 0.1f v in fp32 (common.h::lrelu) and ONE round-to-nearest-even conversion to fp16
        (dst32: none), repeated here in torch float32.  The fused max-pool is exact on the rounded values: the whole wide tensor."""
        assert self.add is None and self.mask is None and not self.upsum_c and not self.urot
        self.ref64(dev)
        pre = self.pre
        assert bool((pre == pre.round()).all()) and float(pre.abs().max()) <= INT_LIMIT, "integer reference: |v| max %g" % float(pre.abs().max())
        slope = torch.tensor(SLOPE, dtype=torch.float32, device=pre.device)
        x = pre.float() + 0.0
        if self.a.act:
            x = torch.where(x > 0, x, x * slope)
        if self.a.dst32:
            return {"dst32": x.permute(0, 3, 1, 2).contiguous()}
        x = x.to(self.dt)

        def wide(t):
            o = torch.full(t.shape[:-1] + (t.shape[-1] + 16,), float("nan"), dtype=self.dt, device=t.device)
            o[..., 8:8 + t.shape[-1]] = t
            return o
        out = {"dst": wide(x)}
        if self.pool:
            out["pool"] = wide(pool_of(x.float().cpu(), self.pool_shifted).to(self.dt).to(x.device))
        return out

    def ints_expected(self, dev=None):
        """the integer operands' expected outputs {name: the whole wide tensor, NaN where the launch stores nothing}, after asserting the
        condition that makes them exact in any accumulation order and in the 16-bit output type: every value, fused 2x2 up-sums included,
        is an integer of magnitude <= INT_LIMIT"""
        assert self.ints
        if len(self.taps) == 1:
            return self._ints_chain(dev)
        if self.a.act or self.a.dst32:
            return self._ints_act(dev)
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


def pool_of(x, shifted):
    """SSDN_OP_POOL_FWD of include/ssdn_hip.h on x [N,H,W,C] (oracle/interp.py::Interp._windows(...).max): 2x2 windows; shifted: of the
    image moved one row down, a zero row on top"""
    from interp import Interp
    return Interp._windows(None, x, shifted).max(3).values


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
    if case.unrot:      # fused UNROT_BWD: ref64 answers in the rotated stack's place; the whole window is written and dst is not touched
        key, Mw = "unrot", M // 4
        assert bool(torch.isnan(got["dst"].float()).all()), "the fused un-rotation stored to dst"
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


def _check_dst32(case, got, dev=None):
    """fp32 NCHW output of fp16 operands: the forward bound of _check_ref; the guards in front of and behind the buffer are still NaN"""
    ref = case.ref64(dev)[0].permute(0, 3, 1, 2)
    tol = 2e-3 * ref.abs() + 2e-3 * float(ref.abs().max()) * 1e-2 + 1e-9
    g = got["dst32"].to(ref.device).double()
    assert bool(torch.isfinite(g).all())
    err = (g - ref).abs()
    assert bool((err <= tol).all()), "dst32: %d elements beyond the bound, max err %.3e" % (int((err > tol).sum()), float(err.max()))
    assert bool(torch.isnan(case.dst32_guards).all()), "stored outside the fp32 output"


def check_pool(case, got):
    """the fused max-pool output is exactly SSDN_OP_POOL_FWD of what the launch itself stored (the max is exact on the rounded values),
    as tests/test_hip_ops.py::test_every_op_teacher_forced has it; the guard channels of its wide tensor are still NaN"""
    M = case.M
    want = pool_of(got["dst"][..., 8:8 + M].float(), case.pool_shifted)
    gp = got["pool"]
    assert torch.equal(gp[..., 8:8 + M].float(), want), "fused max-pool differs from pool(dst) in %d elements" % int((gp[..., 8:8 + M].float() != want).sum())
    assert bool(torch.isnan(gp[..., :8].float()).all()) and bool(torch.isnan(gp[..., 8 + M:].float()).all())


def _check_next32(case, got, dev=None):
    """the second layer's fp32 NCHW output against float64 on the first layer's own stored 16-bit output: the forward bound of _check_ref
    (as tests/test_hip_conv_route.py::_check_dst32); the guards in front of and behind it are still NaN"""
    if dev is not None:
        got = {k: v.to(dev) for k, v in got.items()}
    ref = case.next_ref64(got["dst"][..., 8:8 + case.M], dev).reshape(-1)
    tol = 2e-3 * ref.abs() + 2e-3 * float(ref.abs().max()) * 1e-2 + 1e-9
    buf = got["next32"]
    g = buf[NEXT_GUARD:NEXT_GUARD + case.next_n].double()
    assert bool(torch.isfinite(g).all())
    err = (g - ref).abs()
    print("  second layer M4 %d: max err / bound %.4f" % (case.next["M4"], float((err / tol).max())))
    assert bool((err <= tol).all()), "next32: %d elements beyond the bound, max err %.3e" % (int((err > tol).sum()), float(err.max()))
    assert bool(torch.isnan(buf[:NEXT_GUARD]).all()) and bool(torch.isnan(buf[NEXT_GUARD + case.next_n:]).all()), "stored outside the output"


def check_ints(case, got, dev=None):
    """bit equality of every 16-bit output -- the whole wide tensor: the window holds the float64 reference cast to the output type, every
    other element (guard channels, the channels that only exist as up-sums, the rows a fused UNROT_FWD leaves empty) is still the NaN it was"""
    want = case.ints_expected(dev)
    if "dst32" in want:
        assert bool(torch.isnan(case.dst32_guards).all()), "stored outside the fp32 output"
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
