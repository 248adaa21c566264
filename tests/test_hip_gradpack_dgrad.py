"""GPU: k_gradpack_dgrad (csrc/gradpack_dgrad.hip) per launch -- SSDN_OP_GRAD_PACK and the data gradient of the narrow net_out layer behind it
as ONE launch, against float64 and against the two separate launches.

The executor fuses the two records that open every backward list (csrc/api.hip); the whole-plan tests only see that through
ssdn_conv_set_chain(0 / 1) bit-identity at shapes with H W a multiple of 256.  Here the list [grad_pack, conv] runs on tensors of its own:
  * both outputs are channel windows of NaN-poisoned wide tensors: the packed bf16 gradient with its zero slots up to 16, and the
    96-channel data gradient; scale_out must read {1, 1};
  * C in {1, 2, 3, 9}: below 8 the upper half-wave packs only zeros;
  * 16x16 N 1 is one full block of eight 32-pixel tiles; 12x12 N 2 is nine tiles -- tile 4 straddles the two images, and the second
    block is one-eighth full and leaves its loop early; 8x4 is a single tile; 64x64 N 4 is many blocks;
  * the masks take both signs;
  * ints: integer-valued gradients |g| <= 8 and weights +-1 -- the sum (|v| <= 128) is exact in any order, and what follows is the fixed
    chain bf16(v), * (mask > 0 ? 1 : 0.1f), bf16, repeated in torch float32: bit equality.  rand: the data-gradient bound of
    conv_case._check_ref.  The packed gradient is a plain round-to-nearest-even conversion: bit equality in both.
The launch counters say that no k_conv launch happened in the fused run and exactly one in the separate run, whose outputs must be
bit-identical."""
import ctypes as C

import pytest
import torch

from conv_case import SLOPE, _bits, _rand, _randint, _same

pytestmark = pytest.mark.gpu

SHAPES = {"16x16n1": (1, 16, 16), "12x12n2": (2, 12, 12), "8x4n1": (1, 8, 4), "64x64n4": (4, 64, 64)}
K_CONV = ("conv_mt3", "conv_mt2", "conv_mt1")


def _lib():
    from ssdn.hip import lib as L
    return L, L.load()


@pytest.fixture(autouse=True)
def chain_reset():
    L, lib = _lib()
    for k in L.PROF.values():
        L.check(lib.ssdn_profile_enable(k, 4))
        L.check(lib.ssdn_profile_set_stride(k, 1))
    yield
    lib.ssdn_conv_set_chain(1)
    for k in L.PROF.values():
        lib.ssdn_profile_enable(k, 0)


def _counts(lib):
    L = _lib()[0]
    out = {}
    for name, k in L.PROF.items():
        ms, n, fl, by = C.c_double(), C.c_longlong(), C.c_double(), C.c_double()
        L.check(lib.ssdn_profile_read(k, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)))
        out[name] = n.value
    return out


class Pair:
    """[SSDN_OP_GRAD_PACK, SSDN_OP_CONV (data gradient 16 -> 96, 1x1)] on tensors of its own"""

    def __init__(self, N, H, W, Cg, ints, seed):
        from ssdn.hip import graph
        L, lib = _lib()
        dev = torch.device("cuda:0")
        gen = torch.Generator().manual_seed(2000 + seed)
        self.N, self.H, self.W, self.C = N, H, W, Cg
        if ints:
            self.g = _randint(gen, (N, Cg, H, W), 8)
            w = torch.randint(0, 2, (1, 96, 16), generator=gen).float() * 2 - 1
        else:
            self.g = _rand(gen, (N, Cg, H, W), 3.0)
            w = _rand(gen, (1, 96, 16), 1.0 / 3.0)
        self.w = w.to(torch.bfloat16)
        self.mask = _rand(gen, (N, H, W, 96)).to(torch.float16)
        self.dg, self.dw = self.g.to(dev), self.w.to(dev)

        def wide(c, dtype, fill=None):
            t = torch.full((N, H, W, c + 16), float("nan"), dtype=dtype)
            if fill is not None:
                t[..., 8:8 + c] = fill
            return t.to(dev)
        self.dmask = wide(96, torch.float16, self.mask)
        self.gz, self.dst = wide(16, torch.bfloat16), wide(96, torch.bfloat16)
        self.scale = torch.full((4,), float("nan"), device=dev)
        self.gmax = torch.zeros(4, dtype=torch.int32, device=dev)
        self.gp = L.GradPackArgs(self.dg.data_ptr(), L.View(self.gz.data_ptr(), 32, 8), N, Cg, H, W, 16, self.gmax.data_ptr(), self.scale.data_ptr())
        a = L.ConvArgs()
        a.src0 = L.View(self.gz.data_ptr(), 32, 8)
        a.c0, a.c1, a.up0, a.N, a.H, a.W, a.ntaps = 16, 0, 0, N, H, W, 1
        a.w, a.M, a.Mpad, a.Ktot = self.dw.data_ptr(), 96, 96, 16
        a.mask = L.View(self.dmask.data_ptr(), 112, 8)
        a.dst = L.View(self.dst.data_ptr(), 112, 8)
        cus = lib.ssdn_device_cus()
        a.ltw, a.lth, a.ltn, a.kc = graph.choose_conv_tile(N, H, W, graph.TAPS_1x1, 16, 96, cus=cus if cus > 0 else 256)
        a.bf16, a.kreal = 1, Cg
        self.a = a

    def launch(self):
        from ssdn.hip.engine import OpList, current_stream
        for t in (self.gz, self.dst, self.scale):
            t.fill_(float("nan"))
        OpList([("grad_pack", self.gp), ("conv", self.a)]).run(current_stream())
        torch.cuda.synchronize()
        return dict(gz=self.gz.cpu().clone(), dst=self.dst.cpu().clone(), scale=self.scale.cpu().clone())

    def packed(self):
        """SSDN_OP_GRAD_PACK: the whole wide tensor [N,H,W,32] -- bf16(g) in slots < C, zeros up to 16, NaN outside the window"""
        want = torch.full((self.N, self.H, self.W, 32), float("nan"), dtype=torch.bfloat16)
        want[..., 8:24] = 0
        want[..., 8:8 + self.C] = self.g.permute(0, 2, 3, 1).to(torch.bfloat16)
        return want

    def ref64(self):
        """(the sum in float64 on the packed bf16 gradient, LeakyReLU' of the mask)"""
        gz = self.packed()[..., 8:24].double()
        return torch.einsum("nyxk,mk->nyxm", gz, self.w.double()[0]), torch.where(self.mask.double() > 0, 1.0, SLOPE)


@pytest.mark.parametrize("operands", ["ints", "rand"])
@pytest.mark.parametrize("Cg", [1, 2, 3, 9])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_gradpack_dgrad(shape, Cg, operands):
    L, lib = _lib()
    N, H, W = SHAPES[shape]
    pair = Pair(N, H, W, Cg, operands == "ints", seed=list(SHAPES).index(shape) * 16 + Cg)
    assert pair.a.kc == 16
    _counts(lib)
    got = pair.launch()
    n = _counts(lib)
    assert not any(n.values()), "launch counters %s: the fused launch is none of the profiled kinds (a k_conv launch: not fused)" % n
    assert got["scale"][:2].tolist() == [1.0, 1.0] and bool(torch.isnan(got["scale"][2:]).all())
    packed = pair.packed()
    bad = _bits(got["gz"]) != _bits(packed)
    assert not bool(bad.any()), "packed gradient: %d of %d elements differ" % (int(bad.sum()), bad.numel())
    v, fac = pair.ref64()
    assert bool(torch.isnan(got["dst"][..., :8].float()).all()) and bool(torch.isnan(got["dst"][..., 104:].float()).all())
    if operands == "ints":
        assert bool((v == v.round()).all()) and float(v.abs().max()) <= 128
        x = (v.float() + 0.0).to(torch.bfloat16)
        x = (x.float() * torch.where(pair.mask.float() > 0, torch.tensor(1.0), torch.tensor(SLOPE, dtype=torch.float32))).to(torch.bfloat16)
        bad = _bits(got["dst"][..., 8:104]) != _bits(x)
        assert not bool(bad.any()), "data gradient: %d of %d elements differ from the exact integers' chain" % (int(bad.sum()), bad.numel())
    else:
        ref = v * fac
        tol = 1.6e-2 * ref.abs() + 1.6e-2 * float(ref.abs().max()) * 1e-2 + 1e-9
        g = got["dst"][..., 8:104].double()
        assert bool(torch.isfinite(g).all())
        err = (g - ref).abs()
        print("gradpack_dgrad %s C %d: max err / bound %.4f" % (shape, Cg, float((err / tol).max())))
        assert bool((err <= tol).all()), "data gradient: %d elements beyond the bound, max err %.3e" % (int((err > tol).sum()), float(err.max()))
    assert bool(torch.isnan(pair.dmask[..., :8].float()).all()) and bool(torch.isnan(pair.dmask[..., 104:].float()).all()), "the mask was written"
    # the two records as two launches: the conversion kernel, then the general kernel
    L.check(lib.ssdn_conv_set_chain(0))
    apart = pair.launch()
    n = _counts(lib)
    assert sum(n[k] for k in K_CONV) == 1 and sum(n.values()) == 1, "launch counters %s: not one k_conv launch" % n
    _same(got, apart, "fused launch against the two separate launches")
