"""CPU: the case table of k_gdma's tile walk and epilogues (tests/test_hip_gdma_walk.py runs it on the GPU), held to what it is there for.

k_gdma (csrc/gemm_dma.hip) serves the 1x1 layers of the posterior head.  It is persistent: grid = min(tiles, compute units) workgroups
walk the 256-pixel tiles blockIdx.x, blockIdx.x + grid, ..., and the two operand rings (depth 3, chunks of 32 input channels) run on as
one chunk stream across the tiles of a workgroup.  A regime of the table names what that walk does on 256 compute units; a variant names
one of the kernel's eleven instantiations (tile width, role, EPI) or a Ktot whose chunk count is no multiple of the ring depth.  Here:
  * every case is routed to k_gdma by the library's own host queries (which answer for 256 compute units without a device), walks as its
    regime says, and where it uses them ssdn_conv_fuses_unrot / ssdn_conv_signs say 1 and the second layer can ride in the launch
    (ssdn_chain_len leaves the two records alone, pair_fusable -- the launch count model the GPU test's counters confirm);
  * the integer operands' references meet the conditions that make bit equality a fair test (conv_case.Case._ints_chain);
  * every 1x1 SSDN_OP_CONV that k_gdma serves in the plans of tests/test_cdma_walk_cpu.py has its class (Ktot, Mpad, role, epilogue flags,
    pair, one tile per workgroup / several equal / ragged) in the table: a plan that grows a new class fails here until a case exists;
  * one control of the checker, and the 2^31 byte-offset boundary of gemm_dma_eligible without a launch."""
import ctypes as C

import pytest
import torch

from conv_case import INT_BIAS, INT_IN, INT_LIMIT, INT_NNZ, Case, check_ints
from test_cdma_walk_cpu import PLANS, _plan_args

CUS = 256           # the compute units the regimes are named for
TILE = 256          # pixels of a tile


def walk(tiles, cus=CUS):
    """what the persistent grid does with `tiles` tiles: the fewest and the most tiles of a workgroup, and how many workgroups have the most"""
    grid = min(tiles, cus)
    per = [(tiles - b + grid - 1) // grid for b in range(grid)]
    return dict(tiles=tiles, grid=grid, lo=min(per), hi=max(per), n_hi=per.count(max(per)))


# regime -> ((N, H, W) of the launch, walk() at 256 CUs).  few, ragged2 and deep: H W is a multiple neither of 256 nor of 32 -- images
# straddle tiles AND the 32 pixels of a wave (the fused second layer divides by H W per lane; with H W a multiple of 32 the image of a
# wave's first pixel would do).  u_*: the fused un-rotation, (B, P, P): at P 4 two images share a wave's 32 pixels, at P 8 a tile holds
# four images, at P 16 one.
REGIMES = {
    "one": ((1, 16, 16), dict(tiles=1, grid=1, lo=1, hi=1, n_hi=1)),
    "few": ((16, 10, 8), dict(tiles=5, grid=5, lo=1, hi=1, n_hi=5)),                         # fewer tiles than workgroups
    "even2": ((32, 64, 64), dict(tiles=512, grid=256, lo=2, hi=2, n_hi=256)),               # two tiles each
    "ragged2": ((16, 257, 16), dict(tiles=257, grid=256, lo=1, hi=2, n_hi=1)),              # workgroup 0 has two tiles, all others one
    "deep": ((2048, 10, 8), dict(tiles=640, grid=256, lo=2, hi=3, n_hi=128)),               # half the grid three tiles, half two
    "u_p4": ((48, 4, 4), dict(tiles=3, grid=3, lo=1, hi=1, n_hi=3)),
    "u_one": ((4, 8, 8), dict(tiles=1, grid=1, lo=1, hi=1, n_hi=1)),
    "u_few": ((20, 8, 8), dict(tiles=5, grid=5, lo=1, hi=1, n_hi=5)),
    "u_ragged": ((257, 16, 16), dict(tiles=257, grid=256, lo=1, hi=2, n_hi=1)),
    "u_p64": ((3, 64, 64), dict(tiles=48, grid=48, lo=1, hi=1, n_hi=48)),
    "u_even2": ((32, 64, 64), dict(tiles=512, grid=256, lo=2, hi=2, n_hi=256)),             # BASELINE config 2's own launch
}

F, D = "fwd", "dgrad"
# variant -> (Case arguments, the k_gdma instantiation: output tile width, f(orward fp16) / t (data gradient, bf16), EPI)
VARIANTS = {
    "fwd384": (dict(role=F, c0=384, M=384), "384f0"),
    "fwd384_sign": (dict(role=F, c0=384, M=384, sign_out=True), "384f16"),
    "fwd384_96": (dict(role=F, c0=384, M=96), "96f0"),
    "fwd96_96": (dict(role=F, c0=96, M=96), "96f0"),
    "dgrad96_384": (dict(role=D, c0=96, M=384), "384t0"),
    "dgrad96_384_mask": (dict(role=D, c0=96, M=384, mask=True), "384t1"),
    "dgrad96_384_masksign": (dict(role=D, c0=96, M=384, mask=True, mask_sign=True), "384t9"),
    "dgrad96_96": (dict(role=D, c0=96, M=96), "96t0"),
    "dgrad96_96_mask": (dict(role=D, c0=96, M=96, mask=True), "96t1"),
    "dgrad384_unrot": (dict(role=D, c0=384, M=384, unrot=True), "384t2"),
    "dgrad384_unrot_smask": (dict(role=D, c0=384, M=384, unrot=True, unrot_smask=True), "384t10"),
    # the 96-wide layer + the narrow layer behind it in one launch (M4 1: the sigma network's head; 9: net_out)
    "pair_m1": (dict(role=F, c0=96, M=96, next=dict(M4=1, bias=True, act=False)), "96f4"),
    "pair_m2": (dict(role=F, c0=96, M=96, next=dict(M4=2, bias=False, act=True)), "96f4"),
    "pair_m3": (dict(role=F, c0=96, M=96, next=dict(M4=3, bias=True, act=True)), "96f4"),
    "pair_m9": (dict(role=F, c0=384, M=96, next=dict(M4=9, bias=True, act=False)), "96f4"),               # (the blind-spot head: 384 -> 96 -> 9)
    "pair_m9_bare": (dict(role=F, c0=96, M=96, next=dict(M4=9, bias=False, act=False)), "96f4"),
    # ring phase: Ktot / 32 chunks on rings of depth 3 -- 4 or 5 chunks start the second tile at stage 1 or 2; 1 or 2 are fewer than the
    # loaders' lead
    "k32_96": (dict(role=F, c0=32, M=96), "96f0"),
    "k64_96": (dict(role=F, c0=64, M=96), "96f0"),
    "k128_96": (dict(role=F, c0=128, M=96), "96f0"),
    "k160_96": (dict(role=F, c0=160, M=96), "96f0"),
    "k128_384_mask": (dict(role=D, c0=128, M=384, mask=True), "384t1"),
}
INSTANTIATIONS = ("384f0", "384f16", "384t0", "384t1", "384t9", "384t2", "384t10", "96f0", "96t0", "96t1", "96f4")      # launch_gemm_dma[_with_next]

PLAIN = ["fwd384", "fwd384_sign", "fwd384_96", "fwd96_96", "dgrad96_384", "dgrad96_384_mask", "dgrad96_384_masksign", "dgrad96_96",
         "dgrad96_96_mask", "pair_m1", "pair_m2", "pair_m3", "pair_m9"]
UNROT = ["dgrad384_unrot", "dgrad384_unrot_smask"]
RING = ["k32_96", "k64_96", "k128_96", "k160_96", "k128_384_mask"]
# the 96-wide ones, one 384-wide forward and one 384-wide data gradient with two and three tiles per workgroup (fwd384 at even2: the
# evaluation plans' class)
BIG = ["fwd384_96", "fwd96_96", "dgrad96_96", "dgrad96_96_mask", "pair_m9", "fwd384_sign", "dgrad96_384_masksign"]
CASES = ([(r, v) for r in ("one", "few", "ragged2") for v in PLAIN] +
         [(r, v) for r in ("u_p4", "u_one", "u_few", "u_ragged", "u_p64") for v in UNROT] + [("u_even2", "dgrad384_unrot_smask")] +
         [(r, v) for r in ("even2", "deep") for v in BIG] + [("even2", "fwd384"), ("even2", "pair_m3"), ("deep", "pair_m1"), ("deep", "pair_m9_bare")] +
         [(r, v) for r in ("deep", "ragged2") for v in RING])
IDS = ["%s-%s-%s" % (r, v, VARIANTS[v][1]) for r, v in CASES]


def make_case(regime, variant, ints, device):
    from ssdn.hip import graph
    (N, H, W), _ = REGIMES[regime]
    return Case(N=N, H=H, W=W, c1=0, up0=False, taps=graph.TAPS_1x1, ints=ints, device=device, seed=CASES.index((regime, variant)),
                **VARIANTS[variant][0])


def _lib():
    from ssdn.hip import lib as L
    return L, L.load()


@pytest.fixture(autouse=True)
def settings_reset():
    yield
    lib = _lib()[1]
    lib.ssdn_conv_set_mode(1)
    lib.ssdn_conv_set_chain(1)


def routed_to_gdma(a):
    """the `predicted` logic of tests/test_hip_conv_route.py: a 1x1 launch whose LDS size is not the one k_conv has for it (mode 0 is
    "k_conv always") goes to k_gdma"""
    L, lib = _lib()
    lds = lib.ssdn_conv_lds_bytes(C.byref(a))
    assert lds > 0, lib.ssdn_last_error()
    L.check(lib.ssdn_conv_set_mode(0))
    lds_k_conv = lib.ssdn_conv_lds_bytes(C.byref(a))
    L.check(lib.ssdn_conv_set_mode(1))
    assert lds_k_conv > 0, lib.ssdn_last_error()
    return a.ntaps == 1 and lds != lds_k_conv


def pair_fusable(a, b):
    """the launch count model of the executor's second fusion (csrc/api.hip; csrc/gemm_dma.hip::gemm_dma_fuses_next): the narrow fp32 layer
    b reads exactly what the 96-wide forward layer a, routed to k_gdma, stores -- the two records are ONE launch.  (The GPU test's launch
    counters hold the library to this.)"""
    if not routed_to_gdma(a) or a.bf16 or a.mask.p or a.unrot.p or a.Mpad != 96 or not a.dst.p:
        return False
    if b.bf16 or b.ntaps != 1 or b.dy[0] or b.dx[0] or b.up0 or b.c1 or b.c0 != 96 or b.Ktot != 96 or b.Mpad != 32 or b.M > 32:
        return False
    if not b.dst32 or b.mask.p or b.add.p or b.pool.p or b.upsum.p or b.unrot.p or not b.w:
        return False
    if (b.src0.p, b.src0.cs, b.src0.co) != (a.dst.p, a.dst.cs, a.dst.co) or (b.N, b.H, b.W) != (a.N, a.H, a.W):
        return False
    return _lib()[1].ssdn_conv_lds_bytes(C.byref(b)) > 0          # (b itself is a valid launch)


def flags(a):
    return (bool(a.mask.p), bool(a.mask_sign), bool(a.sign_out), bool(a.unrot.p), bool(a.unrot_smask))


def gdma_class(a, pair):
    w = walk(a.N * a.H * a.W // TILE)
    kind = "one" if w["hi"] == 1 else ("equal" if w["lo"] == w["hi"] else "ragged")
    return (a.Ktot, a.Mpad, D if a.bf16 else F, flags(a), bool(pair), kind)


def table_class(regime, variant):
    """the class of a case of the table from its definition (the parametrised test holds the built arguments to it)"""
    kw, w = VARIANTS[variant][0], REGIMES[regime][1]
    kind = "one" if w["hi"] == 1 else ("equal" if w["lo"] == w["hi"] else "ragged")
    fl = tuple(bool(kw.get(k)) for k in ("mask", "mask_sign", "sign_out", "unrot", "unrot_smask"))
    return (kw["c0"], kw["M"], kw["role"], fl, "next" in kw, kind)


def test_table_runs_all_eleven_instantiations():
    assert {VARIANTS[v][1] for _, v in CASES} == set(INSTANTIATIONS) and len(INSTANTIATIONS) == 11
    assert {v for _, v in CASES} == set(VARIANTS) and len(set(CASES)) == len(CASES)


@pytest.mark.parametrize("regime,variant", CASES, ids=IDS)
def test_case_is_routed_to_k_gdma_walks_its_regime_and_its_integer_reference_is_exact(regime, variant):
    from ssdn.hip.engine import OpList
    L, lib = _lib()
    (N, H, W), want = REGIMES[regime]
    case = make_case(regime, variant, ints=True, device=False)
    a = case.a
    assert routed_to_gdma(a), "the queries do not route the case to k_gdma"
    assert gdma_class(a, case.next is not None) == table_class(regime, variant)
    assert N * H * W % TILE == 0 and walk(N * H * W // TILE) == want
    if any(getattr(a, k) for k in ("sign_out", "mask_sign")):
        assert lib.ssdn_conv_signs(C.byref(a)) == 1
    if case.unrot:
        assert lib.ssdn_conv_fuses_unrot(C.byref(a)) == 1
    if case.next is not None:
        ol = OpList([("conv", a), ("conv", case.a4)])
        assert lib.ssdn_chain_len(ol.arr, 2) == 0          # no chained launch claims the two records ...
        assert pair_fusable(a, case.a4)                     # ... and the second rides in the first one's launch
    # every channel of the weights is hit by several rows; the operands are integers within their bounds, so every sum is an exact
    # integer <= 2 INT_NNZ + 4 whatever the order
    assert int(case.w_hits.min()) >= 2
    l1 = case.w.float().abs().sum((0, 2))
    for t, lim in ((case.s0, INT_IN), (case.w, 1), (case.bias, INT_BIAS)):
        if t is not None:
            assert bool((t.float() == t.float().round()).all()) and float(t.float().abs().max()) <= lim
    assert float(l1.max()) == INT_NNZ and INT_IN * INT_NNZ + INT_BIAS == 68 <= INT_LIMIT
    if case.next is not None:
        assert float(case.w4.float().abs().sum((0, 2)).max()) == INT_NNZ and not a.act
    if N * H * W <= 20000:           # (the larger ones: on the device, in the GPU test)
        want_out = case.ints_expected()
        for k, t in want_out.items():
            lim = INT_NNZ * 68 + INT_BIAS if k == "next32" else INT_LIMIT
            written = t[~t.isnan()].float()
            assert written.numel() == 0 and k == "dst" and case.unrot or float(written.abs().max()) <= lim
        # both signs reach the epilogue: a LeakyReLU or a mask that was ignored would show
        assert float(case.pre.min()) < 0 < float(case.pre.max())
    for m in (case.mask, case.unrot_mask):
        if m is not None:
            assert 0.3 < float((m > 0).float().mean()) < 0.7


def test_every_1x1_class_of_the_plans_has_a_case():
    """the classes of the table against every launch of the plans that k_gdma serves"""
    from ssdn.hip.graph import NetPlan
    table = {table_class(r, v) for r, v in CASES}
    for cin, cout, bs, Bn, H, W, train in PLANS:
        plan = NetPlan("m/", cin, cout, bs, Bn, H, W, cus=CUS, dev_cus=CUS, train=train)
        served = 0
        for lst in (plan.fwd, plan.bwd):
            for i, op in enumerate(lst):
                if op.type != "conv" or len(op.a["taps"]) != 1:
                    continue
                a = _plan_args(plan, op.a)
                if not routed_to_gdma(a):
                    continue
                served += 1
                pair = i + 1 < len(lst) and lst[i + 1].type == "conv" and pair_fusable(a, _plan_args(plan, lst[i + 1].a))
                assert gdma_class(a, pair) in table, "plan %s, %s %s: no case runs k_gdma as this launch does: %s" % (
                    (cin, cout, bs, Bn, H, W, train), op.a["layer"], op.a["role"], gdma_class(a, pair))
        assert served >= 2


def test_checker_tells_two_rotations_apart():
    """control: the un-rotation expectation with the channel blocks 1 and 3 exchanged fails check_ints against the true one -- operands
    that could not tell two rotations apart would make the GPU test worthless"""
    case = make_case("u_few", "dgrad384_unrot", ints=True, device=False)
    true = case.ints_expected()
    check_ints(case, {k: v.clone() for k, v in true.items()})
    B = case.N
    swapped = true["unrot"].clone()
    swapped[B:2 * B], swapped[3 * B:] = true["unrot"][3 * B:], true["unrot"][B:2 * B]
    with pytest.raises(AssertionError, match="unrot"):
        check_ints(case, dict(true, unrot=swapped))
    # ... and so does a zero row in another place than row P-1
    rolled = torch.roll(true["unrot"], 1, 1)
    with pytest.raises(AssertionError, match="unrot"):
        check_ints(case, dict(true, unrot=rolled))


def test_byte_offset_boundary_of_the_route():
    """gemm_dma_eligible bounds pixels * widest channel stride * 2 bytes below 2^31 (32-bit buffer offsets): one tile below the limit
    the launch is still k_gdma's, one tile above it is not (no launch: host queries on dummy addresses)"""
    from ssdn.hip import graph
    case = Case("fwd", 300, 96, 0, False, 96, graph.TAPS_1x1, device=False)       # (300 tiles: a tiling for more tiles than CUs)
    a = case.a
    cs = max(a.src0.cs, a.dst.cs)
    tiles = (2 ** 31 - 1) // (cs * 2 * TILE)
    assert a.H * a.W == TILE and tiles * TILE * cs * 2 < 2 ** 31 <= (tiles + 1) * TILE * cs * 2
    a.N = tiles
    assert routed_to_gdma(a)
    a.N = tiles + 1
    assert not routed_to_gdma(a)
