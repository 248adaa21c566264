"""CPU: the case table of k_cdma's tile walk (tests/test_hip_cdma_walk.py runs it on the GPU), held to the regimes it is there for.

k_cdma (csrc/conv_dma.hip) is persistent: a workgroup walks work items -- `tps` consecutive 16x16 tiles of one strip (image, tile column) --
and, out of tiles, moves on to a further item.  Which of that code a launch runs is decided by the host arithmetic behind
ssdn_conv_dma_split, which answers for 256 compute units where there is no device.  Here:
  * every case of the table reaches its regime (tps, segs, xcd_map, nitems - grid) by the library's own answer;
  * the integer operands' reference of every case meets the condition that makes bit equality a fair test (conv_case.Case.ints_expected);
  * every SSDN_OP_CONV that k_cdma serves in BASELINE config 2's training plan and in the evaluation plans (512x512, 768x768, 352x512 and its
    transpose) has its class (tps > 3, nitems > grid, xcd_map) in the table: a plan that grows a new regime fails here until a case exists."""
import ctypes as C

import pytest

from conv_case import INT_LIMIT, Case

# regime -> ((N, H, W), ssdn_conv_set_mode, what ssdn_conv_dma_split must say at 256 CUs).  Mode 2: too few tiles for the default rule.
# The *_s shapes are the same walks at a size the default rule takes: the library reads / writes sign bytes only there (conv_dma_signs).
REGIMES = {
    "long1": ((2, 80, 16), 2, dict(tiles_x=1, segs=1, tps=5, nitems=2, xcd_map=0)),           # long odd strip, one tile column
    "long3": ((3, 176, 48), 2, dict(tiles_x=3, segs=1, tps=11, nitems=9, xcd_map=0)),         # long strip, reciprocal of 3
    "seg": ((1, 320, 32), 2, dict(segs=4, tps=5, nitems=8, xcd_map=1)),                       # segments of a non-power-of-two length
    "long1_s": ((26, 80, 16), 1, dict(tiles_x=1, segs=1, tps=5, nitems=26, xcd_map=0)),
    "long3_s": ((4, 176, 48), 1, dict(tiles_x=3, segs=1, tps=11, nitems=12, xcd_map=0)),
    "seg_s": ((4, 320, 32), 1, dict(segs=4, tps=5, nitems=32, xcd_map=1)),
    "long5sq": ((4, 80, 80), 2, dict(tiles_x=5, segs=1, tps=5, nitems=20, xcd_map=0)),        # fused UNROT_FWD: H == W, N % 4 == 0
    "short": ((2, 32, 64), 2, dict(segs=2, tps=1, nitems=16, xcd_map=1)),                     # (what the per-op tests already reach)
    "base": ((128, 64, 64), 1, dict(segs=1, tps=4, nitems=512, xcd_map=1, extra=0)),          # BASELINE's own walk
    "second_xcd": ((65, 16, 128), 1, dict(tps=1, nitems=520, xcd_map=1, extra=8)),            # second item, per-XCD ranges
    "second_flat": ((129, 16, 64), 1, dict(tps=1, nitems=516, xcd_map=0, extra=4)),           # second item, flat stride
    "second_deep": ((65, 48, 128), 1, dict(tps=3, nitems=520, xcd_map=1, extra=8)),           # second item behind a walk of several tiles
    "second_long": ((65, 64, 128), 1, dict(tps=4, nitems=520, xcd_map=1, extra=8)),           # ... of more than three (768x768 evaluation)
}

B, P = "blind", "plain"
# variant -> (Case arguments, taps, k_cdma instantiation(s) (MT, BF, EPI, KIND), launches counted as (k_cdma<3>, k_cdma<2 / 1>))
VARIANTS = {
    "fwd96": (dict(role="fwd", c0=96, c1=0, up0=False, M=96), B, "3f0k1", (1, 0)),
    "fwd48": (dict(role="fwd", c0=48, c1=0, up0=False, M=96), B, "3f0k1", (1, 0)),
    "fwd144": (dict(role="fwd", c0=96, c1=48, up0=False, M=96), B, "3f0k1", (1, 0)),                         # three chunks
    "dgrad96_mask_add": (dict(role="dgrad", c0=96, c1=0, up0=False, M=96, mask=True, add=True), B, "3t3k1", (1, 0)),
    "dgrad48_mask_add": (dict(role="dgrad", c0=48, c1=0, up0=False, M=96, mask=True, add=True), P, "3t3k1", (1, 0)),
    "fwd48_m48": (dict(role="fwd", c0=48, c1=0, up0=False, M=48), B, "2f0k1", (0, 1)),
    "fwd16_m48": (dict(role="fwd", c0=16, c1=0, up0=False, M=48), P, "2f0k0", (0, 1)),                       # the general form
    "fwd112up": (dict(role="fwd", c0=96, c1=16, up0=True, M=96), B, "3f0k2", (1, 0)),
    "fwd112up_sign": (dict(role="fwd", c0=96, c1=16, up0=True, M=96, sign_out=True), B, "3f16k2", (1, 0)),
    "fwd96_urot": (dict(role="fwd", c0=96, c1=0, up0=False, M=96, urot=True, urot_smask=True), B, "3f8k1", (1, 0)),
    "fwd96_sign": (dict(role="fwd", c0=96, c1=0, up0=False, M=96, sign_out=True), P, "3f16k1", (1, 0)),
    "dgrad48_m48": (dict(role="dgrad", c0=48, c1=0, up0=False, M=48), B, "2t0k1", (0, 1)),
    "dgrad48_m48_add": (dict(role="dgrad", c0=48, c1=0, up0=False, M=48, add=True), B, "2t2k1", (0, 1)),
    "dgrad48_m48_masksign": (dict(role="dgrad", c0=48, c1=0, up0=False, M=48, mask=True, mask_sign=True), B, "2t33k1", (0, 1)),
    "dgrad96_m144_upsum": (dict(role="dgrad", c0=96, c1=0, up0=False, M=144, upsum_c=96), B, "3t4k1+2t0k1", (1, 1)),    # two blocks: 96 + 64
    "dgrad96_m144_upsum_sign": (dict(role="dgrad", c0=96, c1=0, up0=False, M=144, upsum_c=96, upsum_mask_sign=True), B, "3t36k1+2t0k1", (1, 1)),
    "dgrad96_masksign": (dict(role="dgrad", c0=96, c1=0, up0=False, M=96, mask=True, mask_sign=True), B, "3t33k1", (1, 0)),
    "fwd48_m192": (dict(role="fwd", c0=48, c1=0, up0=False, M=192), P, "3f0k1x2", (2, 0)),                   # two blocks: m_base = 96
    "fwd144up": (dict(role="fwd", c0=96, c1=48, up0=True, M=96), B, "3f0k1", (1, 0)),                        # the halo-row offset advances every other row
}

SMALL = ["fwd96", "dgrad96_mask_add", "fwd48_m48", "fwd16_m48", "fwd112up", "dgrad48_m48", "dgrad48_m48_add", "dgrad96_m144_upsum",
         "fwd48_m192", "fwd144up"]
SIGNS = ["fwd112up_sign", "fwd96_sign", "dgrad48_m48_masksign", "dgrad96_m144_upsum_sign", "dgrad96_masksign"]
CASES = ([(r, v) for r in ("long1", "long3", "seg") for v in SMALL] +
         [(r, v) for r in ("long1_s", "long3_s", "seg_s") for v in SIGNS] +
         [("long5sq", "fwd96_urot"), ("short", "fwd96"), ("short", "dgrad96_mask_add"), ("base", "fwd48"), ("base", "dgrad48_mask_add")] +
         [(r, v) for r in ("second_xcd", "second_flat", "second_deep") for v in ("fwd48", "dgrad48_mask_add", "fwd144")] +
         [("second_long", "fwd48"), ("second_long", "dgrad48_mask_add")])
IDS = ["%s-%s-%s" % (r, v, VARIANTS[v][2]) for r, v in CASES]


def make_case(regime, variant, ints, device):
    from ssdn.hip import graph
    (N, H, W), _, _ = REGIMES[regime]
    kw, taps, _, _ = VARIANTS[variant]
    return Case(N=N, H=H, W=W, taps=graph.TAPS_BLIND if taps == B else graph.TAPS_PLAIN, cm=True, ints=ints, device=device,
                seed=CASES.index((regime, variant)), **kw)


def regime_reached(split, want):
    """what is wrong with the split the library reports, or None"""
    got = dict(split, extra=split["nitems"] - split["grid"])
    bad = {k: (got[k], v) for k, v in dict(want, extra=want.get("extra", 0)).items() if got[k] != v}
    return "split %s: (got, wanted) %s" % (split, bad) if bad else None


def walk_class(split):
    return (split["tps"] > 3, split["nitems"] > split["grid"], split["xcd_map"])


def table_classes():
    """the classes of the table, from what each regime must be (the first test holds every case to that)"""
    return {(w["tps"] > 3, w.get("extra", 0) > 0, w["xcd_map"]) for _, _, w in REGIMES.values()}


@pytest.fixture(autouse=True)
def mode_reset():
    yield
    from ssdn.hip import lib as L
    L.load().ssdn_conv_set_mode(1)


@pytest.mark.parametrize("regime,variant", CASES, ids=IDS)
def test_case_reaches_its_regime_and_its_integer_reference_is_exact(regime, variant):
    from ssdn.hip import lib as L
    lib = L.load()
    _, mode, want = REGIMES[regime]
    L.check(lib.ssdn_conv_set_mode(mode))
    case = make_case(regime, variant, ints=True, device=False)
    served, split = case.split()
    assert served == 1, "k_cdma would not serve the launch"
    assert regime_reached(split, want) is None, regime_reached(split, want)
    assert split["mt_blocks"] == sum(VARIANTS[variant][3])
    if any(getattr(case.a, k) for k in ("sign_out", "mask_sign", "upsum_mask_sign")):
        assert lib.ssdn_conv_signs(C.byref(case.a)) == 1
    if case.urot:
        assert lib.ssdn_conv_fuses_urot(C.byref(case.a)) == 1
    if case.upsum_c:
        assert lib.ssdn_conv_fuses_upsum(C.byref(case.a)) == 1
    # every (tap, channel) position of the weights is hit by several rows, and the reference is made of integers <= INT_LIMIT
    assert int(case.w_hits.min()) >= 2
    want_out = case.ints_expected()
    assert all(float(t[~t.isnan()].float().abs().max()) <= INT_LIMIT for t in want_out.values())


def test_chunk_major_copy_of_the_builder():
    """the chunk-major weight copy Case hands the launch (tests/optim_ref.py::chunk_major_positions) is, for whole 48-channel chunks, the
    permutation tests/test_hip_conv16.py wrote inline before the builder moved, and complete with a 16-channel tail chunk"""
    import torch
    from ssdn.hip import graph
    case = Case("fwd", 3, 96, 48, True, 96, graph.TAPS_BLIND, seed=31, cm=True, device=False)
    nch = case.Ktot // 48
    src = case.w.view(torch.int16).reshape(9, case.Mpad, nch, 6, 8).permute(0, 2, 1, 3, 4)
    pc = torch.arange(6)[None, :] ^ ((torch.arange(case.Mpad)[:, None] >> 3) & 1)
    wc = torch.zeros(9, nch, case.Mpad, 6, 8, dtype=torch.int16)
    wc[:, :, torch.arange(case.Mpad)[:, None], pc] = src
    assert torch.equal(wc.reshape(-1), case.wc)
    # a 16-channel tail chunk: every element of the shadow is in the copy exactly once
    tail = Case("fwd", 1, 96, 16, True, 96, graph.TAPS_BLIND, seed=3, cm=True, device=False)
    assert torch.equal(tail.wc.sort().values, tail.w.view(torch.int16).reshape(-1).sort().values)


PLANS = [(3, 9, True, 32, 64, 64, True), (3, 9, True, 1, 512, 512, False), (3, 9, True, 1, 768, 768, False), (3, 3, False, 1, 352, 512, False),
         (3, 3, False, 1, 512, 352, False)]


def _plan_args(plan, a):
    """dummy addresses, the plan's own strides, and the chunk-major weight copy where the plan has one"""
    from gen_golden_routes import plan_args
    return plan_args(plan, a)


@pytest.mark.parametrize("cin,cout,bs,Bn,H,W,train", PLANS)
def test_every_walk_class_of_the_plans_has_a_case(cin, cout, bs, Bn, H, W, train):
    from ssdn.hip import lib as L
    from ssdn.hip.graph import NetPlan
    lib = L.load()
    table = table_classes()
    plan = NetPlan("m/", cin, cout, bs, Bn, H, W, cus=256, dev_cus=256, train=train)
    served = 0
    for op in plan.fwd + plan.bwd:
        if op.type != "conv":
            continue
        out = (C.c_int32 * 8)()
        rc = lib.ssdn_conv_dma_split(C.byref(_plan_args(plan, op.a)), out)
        assert rc >= 0, lib.ssdn_last_error()
        if rc == 1:
            served += 1
            split = dict(zip(("tiles_x", "tiles_y", "segs", "tps", "nitems", "grid", "xcd_map", "mt_blocks"), out))
            assert walk_class(split) in table, "%s %s (%d, %d, %d): no case walks k_cdma as this launch does: %s" % (
                op.a["layer"], op.a["role"], op.a["N"], op.a["H"], op.a["W"], split)
    assert served >= 6


def test_split_query_answers():
    """invalid arguments: < 0 and a message; mode 0 (k_conv always): 0, with the split k_cdma would have had"""
    from ssdn.hip import lib as L
    lib = L.load()
    bad = L.ConvArgs()
    out = (C.c_int32 * 8)()
    assert lib.ssdn_conv_dma_split(C.byref(bad), out) < 0 and b"ntaps" in lib.ssdn_last_error()
    assert lib.ssdn_conv_dma_split(None, out) < 0
    case = make_case("base", "fwd48", ints=True, device=False)
    assert case.split()[0] == 1
    L.check(lib.ssdn_conv_set_mode(0))
    served, split = case.split()
    assert served == 0 and regime_reached(split, REGIMES["base"][2]) is None
    L.check(lib.ssdn_conv_set_mode(1))
    small = make_case("long1", "fwd96", ints=True, device=False)
    assert small.split()[0] == 0          # too few tiles for the default rule
    L.check(lib.ssdn_conv_set_mode(2))
    assert small.split()[0] == 1
