"""CPU: the case table of SSDN_OP_WGRAD (tests/wgrad_case.py; tests/test_hip_wgrad.py runs it on the GPU), held to what it is there for.

Which instance of the weight-gradient body a launch runs -- (MT, CPW, NL, BOTH, PS, KS, RWX, RWD), the synchronous mode, k_wgrad_thin -- is
decided by host arithmetic on the tile, the strides, the rows per wave and ntiles > nslabs, not by the image size: ssdn_wgrad_variant
reports it without a device.  Here:
  * every row of the table reaches the class it is there for, by the library's own answer, with a tiling ssdn_wgrad_lds_bytes accepts;
  * the generators are fair: their exactness conditions hold for every row, fp32 sums in two pixel orders equal the float64 one, and the
    bf16 rounding of the reference equals an integer model of round-to-nearest-even on every fp16 pattern;
  * the generators can tell: six wrong references differ from the right one under the generators that are there to catch them;
  * every SSDN_OP_WGRAD of the training plans of BASELINE configs 2 to 5 has its class -- (out9, column groups, mblocks, up0, several
    tiles per workgroup, several images per tile) -- in the table: a plan that grows a new class fails here until a row exists."""
import ctypes as C

import numpy as np
import pytest
import torch

import wgrad_case as WC
from wgrad_case import MUTANTS, NAMES, TABLE, make, want_out9


@pytest.fixture(scope="module")
def cases():
    """the GPU-free case of every (row, generator), built once"""
    cache = {}

    def get(name, gen):
        if (name, gen) not in cache:
            cache[(name, gen)] = make(name, gen, device=False)
        return cache[(name, gen)]
    return get


def items(case):
    """csrc/wgrad_body.h::wgrad_items restated: (rows of the input halo / of dz a wave stages per tile, NL, BOTH, sync)"""
    TW, TH, TN = case.TW, case.TH, case.TN
    dys, dxs = [t[0] for t in case.taps] + [0], [t[1] for t in case.taps] + [0]
    HH, HW = TH - min(dys) + max(dys), TW - min(dxs) + max(dxs)
    ix, idz = (HW * (case.Ktot // 8) + 63) // 64, (TW * (case.M // 8) + 63) // 64
    rswx, rswd = (TN * HH + 3) // 4, (TN * TH + 3) // 4
    steps, single = (TN * TH * TW >> 4) - 2, case.ntiles <= case.nslabs
    if idz > 3:
        return rswx, rswd, 99, 0, 0
    if ix <= 4 and (single or rswx + rswd <= steps):
        return rswx, rswd, 4, 0, 0
    if ix <= 6 and (single or (rswx <= steps and rswd <= steps)):
        return rswx, rswd, 6, 1, 0
    if ix <= 6:
        return (rswx, rswd, 4, 0, 1) if ix <= 4 else (rswx, rswd, 6, 1, 1)
    return rswx, rswd, 99, 0, 0


@pytest.mark.parametrize("name", NAMES)
def test_row_reaches_its_class(name, cases):
    from ssdn.hip import lib as L
    lib = L.load()
    case = cases(name, "ints")
    assert case.lds_bytes() >= 0, lib.ssdn_last_error()
    inst, out9 = case.variant()
    want = want_out9(name)
    assert out9[:len(want)] == want, "%s: the library runs %s, the row is there for %s" % (name, out9, want)
    if want[0] == 1:
        assert inst == 100 + want[1] and case.thin and 1 <= case.kreal <= 3
        return
    assert not case.thin
    rswx, rswd, nl, both, sync = items(case)
    assert sync == int(TABLE[name]["sync"]), "%s: synchronous mode %d by the restated wgrad_items" % (name, sync)
    if out9[5]:          # a static schedule: its rows per wave are template arguments
        assert out9[7:] == (rswx, rswd)
    if sync:
        # the library's side of it: the tiling is accepted, runs the generic instance although a workgroup owns several tiles, and the
        # same tiling with 21 accumulators -- which have no synchronous mode -- is refused for that reason
        assert out9[5:] == (0, 0, 0, 0) and case.ntiles > case.nslabs
        N, H, W = TABLE[name]["NHW"]
        big = WC.WCase(case.taps, case.coff, 96, 0, False, N, H, W, 96, case.tile, case.nslabs, device=False)
        if items(big)[4]:
            out = (C.c_int32 * 9)()
            assert lib.ssdn_wgrad_variant(C.byref(big.a), out) < -1 and b"synchronous" in lib.ssdn_last_error()
    if name in ("empty", "thin_empty"):
        assert case.nslabs > case.ntiles
    if name == "g3_partial":      # 28 column tiles in groups of 12: the last group has 4
        assert case.ntaps * (case.Kpad // 32) + 1 == 28 and 4 * out9[2] == 12


def test_needed_classes_are_all_there(cases):
    """the three static schedules, NL = 2, both BOTH forms, sync, column groups with a partial last group, mblocks = 4, up0, several images
    per tile with a ragged last one, thin MT 1 / 2 / 3 on either source, an empty share"""
    keys = {n: cases(n, "ints").plan_key() for n in NAMES}
    o9 = {k[0] for k in keys.values()}
    assert {(o[5], o[6]) for o in o9} >= {(192, 8), (64, 16), (832, 4), (0, 0)}
    assert any(o[3] == 2 for o in o9) and any(o[4] == 1 and o[5] == 0 for o in o9) and any(o[4] == 1 and o[5] == 832 for o in o9)
    assert any(TABLE[n]["sync"] for n in NAMES) and TABLE["g3_partial"]["kw"]["csplit"] == 3 and TABLE["st4b_mb4"]["kw"]["mblocks"] == 4
    assert any(k[3] for k in keys.values()) and any(k[5] and cases(n, "ints").N % cases(n, "ints").TN for n, k in keys.items())
    assert {o[1] for o in o9 if o[0] == 1} == {1, 2, 3} and TABLE["thin_src1"]["src1"]
    assert any(cases(n, "ints").nslabs > cases(n, "ints").ntiles for n in NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_generators_are_fair(name, cases):
    """expected() asserts the exactness conditions of ints, round and probe (and probe's expectation equals the one read straight off the
    source); fp32 sums -- pixels in natural order, and in chunks of 16 from the last to the first -- equal the float64 sum bit for bit"""
    for gen in ("ints", "round", "probe"):
        case = cases(name, gen)
        E, Eb, _ = case.expected()
        for order in (None, "rev16"):
            e32, b32, _ = case.evaluate(dtype=torch.float32, order=order)
            assert torch.equal(e32.double(), E) and torch.equal(b32.double(), Eb), "%s %s: the fp32 sum (order %s) is not the float64 one" % (name, gen, order)
    E, _, A = cases(name, "rand").expected()
    assert bool((E.abs() <= A).all()) and float(A.max()) > 0          # (a tap that never reaches the image: bound 0, the sum is exactly 0)


def test_probe_looks_where_kernels_go_wrong(cases):
    """ragged: the corners, both sides of every seam, the last pixel of the ragged tile and the last image; tn2_ragged: the image seams"""
    px = cases("ragged", "probe").pixels
    assert {(0, 0, 0), (0, 0, 39), (0, 23, 0), (0, 23, 39), (2, 23, 39)} <= set(px)
    for s in (16, 32):
        assert any(x == s for _, _, x in px) and any(x == s - 1 for _, _, x in px)
    for s in (8, 16):
        assert any(y == s for _, y, _ in px) and any(y == s - 1 for _, y, _ in px)
    assert len(px) <= 96
    assert {(1, 0, 0), (2, 0, 0), (1, 7, 7), (4, 7, 7)} <= set(cases("tn2_ragged", "probe").pixels)
    # the storage edges sit in the last 8 channels and hold what they say
    src = cases("st8", "probe").src
    vals = set(src[..., 88:].numpy().view(np.uint16).reshape(-1).tolist())
    assert vals == set(WC.EDGES)
    m8 = cases("m8_k8", "probe")
    assert len(m8.probe_of) == 8 and m8.edge_lo == 8


def test_bf16_rounding_of_the_reference_is_round_to_nearest_even():
    """all 65536 fp16 patterns, NaN excluded: the rounding expected() uses against the integer model on the fp32 bits"""
    bits = np.arange(65536, dtype=np.uint16)
    h = torch.from_numpy(bits.view(np.float16).copy())
    ok = ~torch.isnan(h)
    ours = WC.bf16_rne(h).float().contiguous().view(torch.int32).numpy().astype(np.uint32) >> 16
    model = WC.bf16_bits_rne_numpy(bits)
    assert np.array_equal(ours[ok.numpy()].astype(np.uint16), model[ok.numpy()])
    # the model by hand: a tie to the even side, a tie to the odd side's neighbour, up into the next binade, a subnormal, the largest value
    for h16, b16 in ((0x3C04, 0x3F80), (0x3C0C, 0x3F82), (0x3FFC, 0x4000), (0x0001, 0x3380), (0x7BFF, 0x4780), (0x8000, 0x8000)):
        assert model[h16] == b16
    # ... and truncation is another function on exactly the patterns with bits behind the kept ones set beyond a tie to even
    tr = (WC.bf16_trunc(h).float().contiguous().view(torch.int32).numpy().astype(np.uint32) >> 16).astype(np.uint16)
    assert tr[0x3C04] == model[0x3C04] and tr[0x3C0C] != model[0x3C0C] and tr[0x3C05] != model[0x3C05]


@pytest.mark.parametrize("name", ["st8", "ragged"])
@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_generators_can_tell(name, mutant, cases):
    for gen in MUTANTS[mutant]:
        case = cases(name, gen)
        E, Eb, _ = case.expected()
        Em, Ebm, _ = case.evaluate(mutant=mutant)
        assert not (torch.equal(Em, E) and torch.equal(Ebm, Eb)), "%s: the %s generator cannot tell the mutant %s" % (name, gen, mutant)
    if mutant == "trunc":
        # ... and the other generators cannot: their source values are bf16 values already, or the mutant is not theirs to catch
        case = cases(name, "ints")
        assert torch.equal(case.evaluate(mutant="trunc")[0], case.expected()[0])


# the training plans of BASELINE configs 2 to 5: (cin, cout, blindspot, B, H, W) -- config 3 trains the sigma network beside config 2's
PLANS = [(3, 9, True, 32, 64, 64), (3, 1, False, 32, 64, 64), (3, 3, False, 32, 64, 64), (3, 9, True, 16, 128, 128)]


def plan_wgrad_args(plan, a):
    """ssdn_wgrad_args of a planned op without a device: dummy addresses, the plan's own strides"""
    from ssdn.hip import lib as L

    def view(v):
        return L.View(0x100000, plan.tensors[v.t].shape[-1], v.co) if v is not None else L.View(None, 0, 0)
    s = L.WgradArgs()
    s.dz, s.src0, s.src1 = view(a["dz"]), view(a["src0"]), view(a["src1"])
    s.c0, s.c1, s.up0, s.N, s.H, s.W, s.ntaps = a["c0"], a["c1"], a["up0"], a["N"], a["H"], a["W"], len(a["taps"])
    for t, (dy, dx) in enumerate(a["taps"]):
        s.dy[t], s.dx[t], s.coff[t] = dy, dx, a["coff"][t]
    s.M, s.Mpad, s.Ktot, s.Kpad, s.nslabs = a["M"], a["Mpad"], a["Ktot"], a["Kpad"], a["nslabs"]
    s.slab = s.bslab = 0x100000
    s.ltw, s.lth, s.ltn = a["ltw"], a["lth"], a["ltn"]
    s.csplit, s.mblocks, s.kreal, s.mega, s.cost = a.get("csplit", 0), a.get("mblocks", 1), a.get("kreal", 0), a.get("mega", 0), a.get("cost", 0.0)
    return s


@pytest.mark.parametrize("cin,cout,bs,B,H,W", PLANS)
def test_every_class_of_the_plans_has_a_row(cin, cout, bs, B, H, W, cases):
    from ssdn.hip import lib as L
    from ssdn.hip.graph import NetPlan
    lib = L.load()
    table = {cases(n, "ints").plan_key() for n in NAMES}
    plan = NetPlan("m/", cin, cout, bs, B, H, W, cus=256, dev_cus=256)
    seen = 0
    for op in plan.bwd:
        if op.type != "wgrad":
            continue
        s = plan_wgrad_args(plan, op.a)
        out = (C.c_int32 * 9)()
        assert lib.ssdn_wgrad_variant(C.byref(s), out) >= -1, lib.ssdn_last_error()
        ntiles = -(-s.W // (1 << s.ltw)) * -(-s.H // (1 << s.lth)) * -(-s.N // (1 << s.ltn))
        key = (tuple(out), s.csplit > 1, s.mblocks > 1, bool(s.up0), ntiles > s.nslabs, s.ltn > 0)
        assert key in table, "%s (%d x %d x %d, %d -> %d): no row of the table runs the weight gradient as this launch does: %s" % (
            op.a["layer"], s.N, s.H, s.W, s.Ktot, s.M, key)
        seen += 1
    assert seen >= 20
