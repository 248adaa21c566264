"""GPU: k_conv16 (csrc/conv16.hip) -- the 96-channel 3x3 layers at 16x16 pixels on a resident half-image tile.

Every launch of the class runs twice from the same NaN-poisoned buffers: on k_conv16 (ssdn_conv_set_conv16(3)) and on the path it
replaces, k_conv's flat path (ssdn_conv_set_conv16(0)).  All outputs must agree bit for bit -- the kernel keeps k_conv's accumulation
order, MFMA instruction and operand roles, and its epilogue arithmetic -- and lie within the teacher-forced bounds of
tests/test_hip_ops.py::test_every_op_teacher_forced of a float64 convolution of the same 16-bit operands.  Launches outside the class
(32x32 pixels, 99 input channels, 48 output channels, fp32 output) must be refused by the predicate and stay what they were; one
Denoiser.train_step with the kernel on and off must leave the same bits everywhere.

The plans hold these launches with the flags used here: forward bias + LeakyReLU; data gradient with the fp16 activation as LeakyReLU' mask
(no launch of k_conv's reads sign bytes: ssdn_conv_signs refuses them, here as before), with the skip addend, and -- decode_block_3.0's --
with the fused SSDN_OP_UPSUM_BWD output, which the library only fuses into a launch without mask and addend (ssdn_conv_fuses_upsum)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SLOPE = 0.1


def _lib():
    from ssdn.hip import lib as L
    return L, L.load()


@pytest.fixture(autouse=True)
def conv16_reset():
    yield
    L, lib = _lib()
    lib.ssdn_conv_set_conv16(-1)
    lib.ssdn_conv_set_mode(1)


def _rand(gen, shape, scale=1.0):
    return (torch.rand(shape, generator=gen) * 2 - 1) * scale


class Case:
    """One SSDN_OP_CONV launch on tensors of its own.  Every tensor is a channel window (co = 8) of a wider one (cs = channels + 16), so a
    stride or offset taken from the wrong view shows."""

    def __init__(self, role, N, c0, c1, up0, M, taps, H=16, W=16, mask=False, add=False, upsum_c=0, bias=None, seed=0, dst32=False,
                 edge=False, cm=False):
        from ssdn.hip.graph import choose_conv_tile
        L, lib = _lib()
        self.role, self.N, self.H, self.W, self.c0, self.c1, self.up0, self.M, self.upsum_c = role, N, H, W, c0, c1, up0, M, upsum_c
        bf = role == "dgrad"
        self.dt = torch.bfloat16 if bf else torch.float16
        self.taps = [(-dy, -dx) for dy, dx in taps] if bf else list(taps)      # the data gradient walks the mirrored window
        self.Ktot, self.Mpad = c0 + c1, (M + 31) // 32 * 32
        gen = torch.Generator().manual_seed(1000 + seed)
        hs, ws = (H // 2, W // 2) if up0 else (H, W)
        self.keep = []

        def view(t):
            """[..., C] -> the device tensor [..., C + 16] that holds it at channel 8, and its ssdn_view"""
            wide = torch.full(t.shape[:-1] + (t.shape[-1] + 16,), float("nan"), dtype=t.dtype)
            wide[..., 8:8 + t.shape[-1]] = t
            d = wide.to(DEV)
            self.keep.append(d)
            return d, L.View(d.data_ptr(), d.shape[-1], 8)

        s0 = _rand(gen, (N, hs, ws, c0)) if c0 else None
        s1 = _rand(gen, (N, H, W, c1)) if c1 else None
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
        w = _rand(gen, (9, self.Mpad, self.Ktot), 1.0 / (3.0 * self.Ktot ** 0.5))
        w[:, M:] = 0
        self.w = w.to(self.dt)
        self.dw = self.w.to(DEV)
        self.bias = _rand(gen, (M,), 0.3) if (bias if bias is not None else not bf) else None
        self.dbias = self.bias.to(DEV) if self.bias is not None else None
        self.mask = _rand(gen, (N, H, W, M)).to(torch.float16) if mask else None
        self.add = _rand(gen, (N, H, W, M)).to(self.dt) if add else None
        self.umask = _rand(gen, (N, H // 2, W // 2, upsum_c)).to(torch.float16) if upsum_c else None

        a = L.ConvArgs()
        if c0:
            _, a.src0 = view(self.s0)
        if c1:
            _, a.src1 = view(self.s1)
        a.c0, a.c1, a.up0, a.N, a.H, a.W, a.ntaps = c0, c1, int(up0), N, H, W, 9
        for t, (dy, dx) in enumerate(self.taps):
            a.dy[t], a.dx[t] = dy, dx
        a.w, a.M, a.Mpad, a.Ktot = self.dw.data_ptr(), M, self.Mpad, self.Ktot
        a.bias = self.dbias.data_ptr() if self.dbias is not None else None
        a.act = int(not bf)
        if mask:
            _, a.mask = view(self.mask)
        if add:
            _, a.add = view(self.add)
        self.outs = {}
        if dst32:
            self.outs["dst32"] = torch.empty(N, M, H, W, device=DEV)
            a.dst32 = self.outs["dst32"].data_ptr()
        else:
            self.outs["dst"], a.dst = view(torch.zeros(N, H, W, M, dtype=self.dt))
        if upsum_c:
            self.outs["upsum"], a.upsum = view(torch.zeros(N, H // 2, W // 2, upsum_c, dtype=self.dt))
            _, a.upsum_mask = view(self.umask)
            a.upsum_c = upsum_c
        a.ltw, a.lth, a.ltn, a.kc = choose_conv_tile(N, H, W, self.taps, self.Ktot, self.Mpad, out16=not dst32, cus=lib.ssdn_device_cus())
        a.bf16, a.kreal = int(bf), self.Ktot
        if cm:
            # the chunk-major copy SSDN_OP_WPACK writes next to the shadow (ssdn_conv_args.wc): [tap][chunk][Mpad][48], the 16-byte piece p
            # of row m at piece p ^ ((m >> 3) & 1)
            nch = self.Ktot // 48
            src = self.w.view(torch.int16).reshape(9, self.Mpad, nch, 6, 8).permute(0, 2, 1, 3, 4)
            pc = torch.arange(6)[None, :] ^ ((torch.arange(self.Mpad)[:, None] >> 3) & 1)                # [m][p] -> stored piece
            wc = torch.zeros(9, nch, self.Mpad, 6, 8, dtype=torch.int16)
            wc[:, :, torch.arange(self.Mpad)[:, None], pc] = src
            self.dwc = wc.to(DEV)
            a.wc = self.dwc.data_ptr()
        self.a = a

    def eligible(self):
        L, lib = _lib()
        return lib.ssdn_conv16_eligible(C.byref(self.a))

    def run(self, roles):
        """the launch with k_conv16 allowed for `roles`, from poisoned outputs -> {name: bits of the whole (wide) output tensor}"""
        from ssdn.hip.engine import OpList, current_stream
        L, lib = _lib()
        L.check(lib.ssdn_conv_set_conv16(roles))
        for t in self.outs.values():
            t.fill_(float("nan"))
        OpList([("conv", self.a)]).run(current_stream())
        torch.cuda.synchronize()
        return {k: t.detach().cpu().clone() for k, t in self.outs.items()}

    def ref64(self):
        """float64 convolution of the 16-bit operands by the formula of include/ssdn_hip.h -> (dst [N,H,W,M], upsum or None)"""
        N, H, W = self.N, self.H, self.W
        parts = []
        if self.c0:
            s = self.s0.double()
            if self.up0:
                s = s.repeat_interleave(2, 1).repeat_interleave(2, 2)
            parts.append(s)
        if self.c1:
            parts.append(self.s1.double())
        x = torch.cat(parts, -1)
        xp = torch.zeros(N, H + 4, W + 4, self.Ktot, dtype=torch.float64)
        xp[:, 2:2 + H, 2:2 + W] = x
        w = self.w.double()
        v = torch.zeros(N, H, W, self.M, dtype=torch.float64)
        for t, (dy, dx) in enumerate(self.taps):
            v += torch.einsum("nyxk,mk->nyxm", xp[:, 2 + dy:2 + dy + H, 2 + dx:2 + dx + W], w[t, :self.M])
        if self.bias is not None:
            v += self.bias.double()
        if self.a.act:
            v = torch.where(v > 0, v, SLOPE * v)
        conv = v.clone()
        if self.add is not None:
            v = v + self.add.double()
        if self.mask is not None:
            v = v * torch.where(self.mask.double() > 0, 1.0, SLOPE)
        up = None
        if self.upsum_c:
            u = v[..., :self.upsum_c]
            g = torch.where(self.umask.double() > 0, 1.0, SLOPE)
            up = (u[:, 0::2, 0::2] + u[:, 0::2, 1::2] + u[:, 1::2, 0::2] + u[:, 1::2, 1::2]) * g
            self.up_abs = (u[:, 0::2, 0::2].abs() + u[:, 0::2, 1::2].abs() + u[:, 1::2, 0::2].abs() + u[:, 1::2, 1::2].abs()) * g
        return v, up, conv


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(new, old, what):
    assert new.keys() == old.keys()
    for k in new:
        diff = _bits(new[k]) != _bits(old[k])
        assert not bool(diff.any()), "%s: %s differs in %d of %d elements" % (what, k, int(diff.sum()), diff.numel())


def _check_ref(case, got, sparse=False):
    """the bounds of test_every_op_teacher_forced: one ulp of the storage type (fp16 2e-3, bf16 1.6e-2) of the element + 1e-2 of that of the
    largest; with an addend one more rounding relative to the addends; the fused up-sum 1.6e-2 of the element + 2e-2 of the mean.
    sparse (the border-values-only inputs, where most up-sums are exactly zero and the mean says nothing about an element's addends): the
    up-sum's bound is what that mean stands for, written out -- each of the four bf16 addends within one bf16 ulp (2^-8) of ITS size, plus
    one ulp of the sum for its own rounding."""
    ref, up, conv = case.ref64()
    M, uc = case.M, case.upsum_c
    ulp = 1.6e-2 if case.role == "dgrad" else 2e-3
    g = got["dst"][..., 8:8 + M].double()
    tol = ulp * ref.abs() + ulp * float(ref.abs().max()) * 1e-2 + 1e-9
    if case.add is not None:
        scale = torch.where(case.mask.double() > 0, 1.0, SLOPE) if case.mask is not None else 1.0
        tol = tol + ulp * (case.add.double().abs() + conv.abs()) * scale
    err = (g - ref).abs()[..., uc:]
    print("%s N %d %d+%d->%d: max err / bound %.4f" % (case.role, case.N, case.c0, case.c1, M, float((err / tol[..., uc:]).max())))
    assert bool(torch.isfinite(g[..., uc:]).all())
    assert bool((err <= tol[..., uc:]).all()), "dst: %d elements beyond the bound, max err %.3e" % (int((err > tol[..., uc:]).sum()), float(err.max()))
    # what the launch does not own stays poisoned: the guard channels, and the channels that only exist as up-sums
    assert bool(torch.isnan(got["dst"][..., :8].float()).all()) and bool(torch.isnan(got["dst"][..., 8 + M:].float()).all())
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


def _taps(name):
    from ssdn.hip import graph
    return graph.TAPS_BLIND if name == "blind" else graph.TAPS_PLAIN


# (role, c0, c1, up0, M, mask, add, upsum_c): the four launches of decode_block_3.0 / 3.2, and the data gradient with mask AND addend
LAUNCHES = {
    "fwd_96_96": ("fwd", 96, 0, False, 96, False, False, 0),
    "fwd_144up_96": ("fwd", 96, 48, True, 96, False, False, 0),
    "dgrad_96_96_mask": ("dgrad", 96, 0, False, 96, True, False, 0),
    "dgrad_96_144_upsum": ("dgrad", 96, 0, False, 144, False, False, 96),
    "dgrad_96_96_mask_add": ("dgrad", 96, 0, False, 96, True, True, 0),
}


def _both(case, what):
    L, lib = _lib()
    L.check(lib.ssdn_conv_set_conv16(3))
    assert case.eligible() == 1, "%s: not claimed by ssdn_conv16_eligible" % what
    new = case.run(3)
    assert case.eligible() == 1
    old = case.run(0)
    assert case.eligible() == 0, "%s: the switch does not reach the old path" % what
    _same(new, old, what)
    return new


@pytest.mark.parametrize("name,taps", [(n, "blind") for n in LAUNCHES] + [("fwd_144up_96", "plain"), ("dgrad_96_144_upsum", "plain")])
def test_conv16_against_k_conv_and_float64(name, taps):
    """N = 3: image and half indices that are no power of two, and a last workgroup group that is partly void.  TAPS_PLAIN once per role."""
    role, c0, c1, up0, M, mask, add, uc = LAUNCHES[name]
    case = Case(role, 3, c0, c1, up0, M, _taps(taps), mask=mask, add=add, upsum_c=uc, seed=len(name))
    _check_ref(case, _both(case, name))


@pytest.mark.parametrize("name", ["fwd_96_96", "fwd_144up_96", "dgrad_96_96_mask", "dgrad_96_144_upsum"])
def test_conv16_chunk_major_weights(name):
    """the plans hand these launches the chunk-major copy of the weights too, and k_conv16 streams from it (contiguous slices); k_conv's
    flat path reads the plain shadow.  Same bits."""
    role, c0, c1, up0, M, mask, add, uc = LAUNCHES[name]
    case = Case(role, 3, c0, c1, up0, M, _taps("blind"), mask=mask, add=add, upsum_c=uc, seed=31, cm=True)
    _check_ref(case, _both(case, name + " (chunk-major weights)"))


@pytest.mark.parametrize("name", ["fwd_144up_96", "dgrad_96_144_upsum", "dgrad_96_96_mask"])
def test_conv16_halo_zero_fill(name):
    """Inputs that are zero except next to the borders the halo zero-fills: rows 0 and 1 in the forward role (the blind-spot window reaches
    two rows up), the last two rows in the data gradient (it reaches two rows down), columns 0 and 15.  A fill that starts a row or a
    column off multiplies exactly these values."""
    role, c0, c1, up0, M, mask, add, uc = LAUNCHES[name]
    case = Case(role, 3, c0, c1, up0, M, _taps("blind"), mask=mask, add=add, upsum_c=uc, seed=77, edge=True)
    _check_ref(case, _both(case, name + " (border values only)"), sparse=True)


@pytest.mark.parametrize("name", ["fwd_96_96", "dgrad_96_144_upsum"])
def test_conv16_single_image(name):
    role, c0, c1, up0, M, mask, add, uc = LAUNCHES[name]
    case = Case(role, 1, c0, c1, up0, M, _taps("blind"), mask=mask, add=add, upsum_c=uc, seed=5)
    _check_ref(case, _both(case, name + " N = 1"))


FALLBACKS = {
    "32x32": dict(role="fwd", N=1, c0=96, c1=0, up0=False, M=96, H=32, W=32),
    "99_channels": dict(role="fwd", N=3, c0=96, c1=16, up0=False, M=96),          # 99 real channels in 112 slots: no whole 48-channel chunks
    "48_outputs": dict(role="fwd", N=3, c0=96, c1=0, up0=False, M=48),
    "dst32": dict(role="fwd", N=3, c0=96, c1=0, up0=False, M=9, dst32=True),
}


@pytest.mark.parametrize("name", list(FALLBACKS))
def test_conv16_refuses_what_is_not_its_class(name):
    """the predicate says no with the kernel switched on, and the launch gives what it gives with the kernel switched off"""
    case = Case(taps=_taps("blind"), seed=11, **FALLBACKS[name])
    L, lib = _lib()
    L.check(lib.ssdn_conv_set_conv16(3))
    assert case.eligible() == 0
    new, old = case.run(3), case.run(0)
    _same(new, old, name)
    key = "dst32" if "dst32" in new else "dst"
    body = new[key] if key == "dst32" else new[key][..., 8:8 + case.M]
    assert bool(torch.isfinite(body.float()).all())


def _train_step_state(roles, accumulate):
    import restate as R
    import ssdn
    from ssdn.denoiser import Denoiser
    from ssdn.datasets import NoisyDataset
    from ssdn.params import ConfigValue, NoiseAlgorithm, NoiseValue
    L, lib = _lib()
    L.check(lib.ssdn_conv_set_conv16(roles))
    cfg = ssdn.cfg.base()
    cfg[ConfigValue.ALGORITHM] = NoiseAlgorithm.SELFSUPERVISED_DENOISING
    cfg[ConfigValue.NOISE_STYLE] = "gauss25"
    cfg[ConfigValue.NOISE_VALUE] = NoiseValue.KNOWN
    ssdn.cfg.infer(cfg, model_only=True)
    d = Denoiser(cfg, device="cuda:0")
    d.get_model(Denoiser.MODEL, parallelised=False).load_state_dict(R.reference_state_dict(R.make_params(3, 9, True, seed=5)))
    d.mark_dirty()
    B, P = 2, 64
    d.train()
    out = None
    for k in range(2 if accumulate else 1):
        clean = R.hash_tensor((B, 3, P, P), 61 + 10 * k, 0, 1)
        noisy = torch.clamp(clean + R.hash_tensor((B, 3, P, P), 62 + 10 * k, -1, 1) * 0.17, 0, 1)
        meta = {NoisyDataset.Metadata.INPUT_NOISE_VALUES: torch.full((B, 1, 1, 1), 25 / 255.0), NoisyDataset.Metadata.CLEAN: clean}
        if accumulate and k == 0:
            d.accumulate_step([noisy, clean, meta])
        else:
            out = d.train_step([noisy, clean, meta], lr=3e-4)
    torch.cuda.synchronize()
    state = {"out/" + str(k): v.detach().cpu().clone() for k, v in out.items() if torch.is_tensor(v)}
    state["flat"] = d.flat.detach().cpu().clone()
    state["flat_grad"] = d.flat_grad.detach().cpu().clone()
    return state


@pytest.mark.parametrize("accumulate", [False, True])
def test_train_step_is_bit_identical_with_conv16_on_and_off(accumulate):
    """batch 2 at 64x64: 8 rotated images whose 16x16 stage is the kernel's class.  The returned dictionary, the flat gradient and the updated
    parameters; once with a micro-batch accumulated in front of the step."""
    on = _train_step_state(3, accumulate)
    off = _train_step_state(0, accumulate)
    assert len(on) >= 3
    _same(on, off, "train_step")
    assert bool(torch.isfinite(on["flat"]).all()) and float(on["flat_grad"].abs().max()) > 0
