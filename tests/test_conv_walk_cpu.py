"""CPU: the case table of k_conv per launch (tests/test_hip_conv_walk.py runs it on the GPU), held to the regimes it is there for.

k_conv<MT, BF, KS, threads> (csrc/conv_mfma.hip) is the kernel SSDN_OP_CONV falls back to: four K loops (pipelined, ASYNC, ALLW, FLAT),
three epilogues (fp32 NCHW, row-wise with buffer resources clipped at the image edge, flat with the fused max-pool and 2x2 up-sum) and 50
instantiations.  Which of that a launch runs is decided by host code -- conv_route, conv_staging, conv_async, the split of the output
channels into launches -- which ssdn_conv_variant reports, for 256 compute units where there is no device.  Here:
  * every case of the table reaches its regime (instantiation, K loop, channel blocks, tiles, first channel of each launch) by the library's
    own answer, with the fusions it asks for;
  * the integer operands' reference of every case meets the conditions that make bit equality a fair test (conv_case.Case.ints_expected);
  * the table reaches every instantiation the library builds, and every residue of the step count mod 6 (the unrolled pipeline's exits)
    among the pipelined and among the ASYNC cases;
  * every class of k_conv launch in BASELINE config 2's training plan, the evaluation plans and a non-square training plan has a case: a
    plan that grows a new class fails here until a case exists.

A regime is written "<MT><f|t><KS>:<threads>:<path>:<nblk>:<tiles>:<m_base>" per launch (f: forward fp16, t: data gradient bf16), launches
joined by "+"."""
import ctypes as C

import pytest

from conv_case import INT_LIMIT, PATHS, Case

B, P, O = "blind", "plain", "1x1"


def fwd(N, H, W, c0, c1, M, up0=False, **kw):
    return dict(role="fwd", N=N, H=H, W=W, c0=c0, c1=c1, up0=up0, M=M, **kw)


def dgrad(N, H, W, c0, c1, M, up0=False, **kw):
    return dict(role="dgrad", N=N, H=H, W=W, c0=c0, c1=c1, up0=up0, M=M, **kw)


# name -> (Case arguments, taps, tile (None: the planner's), ssdn_conv_set_mode, the regime ssdn_conv_variant must answer at 256 CUs).
# Mode 1 wherever the route itself gives k_conv; mode 0 ("k_conv always") only where k_cdma / k_gdma / k_conv16 would take the shape.
CASES = {
    # ---- pipelined, blocks of 96 (+ 64 / 32) output channels, the row-wise epilogue -------------------------------------------------------
    # tile smaller than the workgroup: surplus lanes compute on pixel 0 and store nothing; all 9 tap rotations; > 256 tiles
    "pipe3-small": (fwd(1, 68, 64, 48, 0, 96), P, (2, 2, 0, 48), 1, "3f3:256:pipe:1:272:0"),
    "pipe3-full": (fwd(5, 128, 128, 48, 0, 96), B, (4, 4, 0, 48), 1, "3f3:256:pipe:1:320:0"),                    # cpp = 12
    "pipe3-rem2": (dgrad(1, 136, 128, 96, 0, 160, mask=True, add=True), B, (3, 3, 0, 32), 1, "3t2:256:pipe:1:272:0+2t2:256:pipe:1:272:96"),
    "pipe3-rem1": (fwd(1, 136, 128, 32, 0, 120), P, (3, 3, 0, 16), 1, "3f1:256:pipe:1:272:0+1f1:256:allw:1:272:96"),    # m_cnt 24: cpp = 3
    # ragged in W, H and N; half-resolution staging; cpp = 9
    "pipe3-ragged-up": (fwd(3, 38, 50, 48, 48, 72, up0=True), B, (2, 2, 1, 48), 1, "3f3:256:pipe:1:260:0"),
    "pipe3-straddle": (fwd(3, 38, 50, 96, 96, 96), P, (2, 2, 1, 64), 1, "3f4:256:pipe:1:260:0"),                  # a chunk of src0 | src1
    "pipe2-m40": (fwd(3, 38, 50, 16, 0, 40), P, (2, 2, 1, 16), 1, "2f1:256:pipe:1:260:0"),                       # cpp = 5
    # what `ssdn eval` runs for a batch of four 480x320 images at the 120x80 stage
    "eval-enc": (fwd(16, 120, 80, 48, 0, 48), B, None, 1, "2f3:256:pipe:1:600:0"),
    "eval-dec": (fwd(16, 120, 80, 96, 48, 96, up0=True), B, None, 1, "3f3:256:pipe:1:600:0"),
    # the head's data gradient into 16 channel slots: one step
    "pipe3-1x1-mask": (dgrad(1, 68, 64, 16, 0, 96, mask=True), O, (2, 2, 0, 16), 1, "3t1:256:pipe:1:272:0"),
    "pipe1-1x1-mask": (dgrad(2, 96, 64, 16, 0, 96, mask=True), O, None, 1, "1t1:256:pipe:3:48:0"),
    # 1x1 layers that may not run ASYNC: an up-sampled source; a chunk that straddles the sources; one chunk; 2, 3, 4, 5 steps
    "pipe-1x1-up": (fwd(3, 10, 18, 64, 32, 96, up0=True), O, (3, 3, 2, 32), 1, "1f2:256:pipe:3:6:0"),
    "pipe-1x1-straddle": (fwd(3, 10, 18, 24, 40, 96), O, (3, 3, 2, 16), 1, "1f1:256:pipe:3:6:0"),
    "pipe-1x1-up5": (fwd(3, 10, 18, 40, 40, 96, up0=True), O, (3, 3, 2, 16), 1, "1f1:256:pipe:3:6:0"),
    "pipe-1x1-up2": (dgrad(3, 10, 18, 48, 48, 96, up0=True), O, (3, 3, 2, 48), 1, "1t3:256:pipe:3:6:0"),
    "pipe-1x1-one": (fwd(3, 10, 18, 64, 0, 96), O, (3, 3, 2, 64), 1, "1f4:256:pipe:3:6:0"),
    # ... a tile whose 16-byte pieces are no whole number of workgroup-wide LDS-DMA instructions (64 pixels x 6 pieces on 256 lanes): run
    # ASYNC, the surplus lanes of the last instruction zeroed the start of the other tile buffer / the first weight rows
    "pipe-1x1-small-tile": (fwd(2, 8, 8, 96, 0, 96), O, (3, 3, 0, 48), 1, "1f3:256:pipe:3:2:0"),
    "pipe-1x1-small-tile3": (fwd(2, 8, 8, 96, 48, 96), O, (3, 3, 0, 48), 1, "1f3:256:pipe:3:2:0"),
    "async3-small-tile": (fwd(2, 8, 8, 96, 0, 96), O, (3, 3, 0, 32), 1, "1f2:256:async:3:2:0"),                  # 64 x 4 pieces: one instruction
    # 3x3 with fp32 NCHW output: never 32-channel blocks, never ALLW
    "pipe1-dst32": (fwd(2, 20, 12, 48, 0, 9, dst32=True), P, (3, 3, 2, 48), 1, "1f3:256:pipe:1:6:0"),
    "pipe3-dst32-rem1": (fwd(3, 16, 16, 96, 0, 100, dst32=True), P, None, 1, "3f3:256:pipe:1:3:0+1f3:256:pipe:1:3:96"),
    # ---- ASYNC: 1x1, the LDS-DMA double buffer --------------------------------------------------------------------------------------------
    "async2-ragged": (fwd(3, 10, 18, 96, 0, 96), O, (4, 4, 0, 48), 1, "1f3:256:async:3:6:0"),                    # out-of-image pixels zero-filled
    "async5-blocks": (fwd(3, 10, 18, 64, 96, 384), O, (3, 3, 2, 32), 1, "1f2:256:async:12:6:0"),                 # tiles % 8 != 0 with 12 blocks
    "async3": (dgrad(3, 10, 18, 96, 0, 96, mask=True), O, (3, 3, 2, 32), 1, "1t2:256:async:3:6:0"),
    "async4": (fwd(3, 10, 18, 64, 0, 160), O, (3, 3, 2, 16), 1, "1f1:256:async:5:6:0"),
    "async7": (fwd(3, 10, 18, 48, 64, 96), O, (3, 3, 2, 16), 1, "1f1:256:async:3:6:0"),
    "async6-dst32-m9": (fwd(2, 10, 18, 96, 0, 9, dst32=True), O, (4, 4, 0, 16), 1, "1f1:256:async:1:4:0"),         # net_out
    "async2-dst32": (fwd(2, 64, 64, 96, 0, 9, dst32=True), O, None, 1, "1f3:256:async:1:32:0"),                 # the plans' net_out launch
    "async3-mt3": (dgrad(1, 68, 64, 96, 0, 160), O, (2, 2, 2, 32), 1, "3t2:256:async:1:272:0+2t2:256:async:1:272:96"),
    # ---- ALLW: 32-channel blocks, all nine weight slices of a chunk next to the tile ------------------------------------------------------
    "allw-ks6": (fwd(2, 32, 32, 96, 0, 96), B, (4, 4, 0, 96), 1, "1f6:256:allw:3:8:0"),
    "allw-ks6-up": (fwd(4, 32, 32, 48, 48, 96, up0=True), B, (4, 4, 0, 96), 1, "1f6:256:allw:3:16:0"),
    "allw-ks6-ragged": (fwd(1, 22, 32, 96, 0, 96), P, None, 1, "1f6:256:allw:3:3:0"),
    "allw-ks6-ragged-up": (fwd(1, 22, 32, 48, 48, 96, up0=True), P, None, 1, "1f6:256:allw:3:3:0"),
    "allw-ragged-up": (fwd(3, 22, 34, 96, 48, 96, up0=True), P, None, 1, "1f3:256:allw:3:15:0"),                 # 3 chunks
    "allw-up": (fwd(4, 32, 32, 96, 48, 96, up0=True), B, (4, 4, 0, 48), 1, "1f3:256:allw:3:16:0"),
    "allw-enc": (fwd(4, 32, 32, 48, 0, 48), B, None, 1, "1f3:256:allw:2:16:0"),
    "allw-enc-ragged": (fwd(1, 44, 64, 48, 0, 48), P, None, 1, "1f3:256:allw:2:12:0"),
    "allw-ks1-up": (fwd(2, 32, 32, 96, 16, 96, up0=True), P, (4, 4, 0, 16), 1, "1f1:256:allw:3:8:0"),
    "allw-m8": (fwd(2, 20, 12, 32, 0, 8), P, None, 1, "1f2:256:allw:1:3:0"),                                     # cpp = 1
    "allw-t3-add": (dgrad(2, 48, 32, 48, 0, 48, add=True), P, None, 1, "1t3:256:allw:2:12:0"),
    "allw-t3-mask": (dgrad(2, 32, 32, 48, 0, 48, mask=True), P, (4, 4, 0, 48), 1, "1t3:256:allw:2:8:0"),
    "allw-t3-ragged": (dgrad(2, 3, 2, 48, 0, 48), P, None, 1, "1t3:256:allw:2:1:0"),
    "allw-t3-ragged-add": (dgrad(2, 12, 8, 48, 0, 48, add=True), P, None, 1, "1t3:256:allw:2:1:0"),
    "allw-t6": (dgrad(2, 48, 32, 96, 0, 144), P, None, 1, "1t6:256:allw:5:12:0"),
    "allw-t6-mask": (dgrad(2, 48, 32, 96, 0, 96, mask=True), P, None, 1, "1t6:256:allw:3:12:0"),
    "allw-t6-ragged": (dgrad(2, 12, 8, 96, 0, 144), P, None, 1, "1t6:256:allw:5:1:0"),
    "allw-t6-ragged-mask": (dgrad(2, 6, 4, 96, 0, 96, mask=True), P, None, 1, "1t6:256:allw:3:1:0"),
    # ---- FLAT: the 256-pixel tile is made of whole images; the fused max-pool and 2x2 up-sum ----------------------------------------------
    "flat-upsum": (dgrad(64, 2, 4, 96, 0, 144, upsum_c=96), B, None, 1, "1t3:256:flat:5:2:0"),                   # H != W at half resolution
    "flat-upsum48": (dgrad(32, 4, 4, 96, 0, 96, upsum_c=48), B, None, 1, "1t3:256:flat:3:2:0"),
    "flat-pool": (fwd(2, 8, 32, 48, 0, 48, pool=True, pool_shifted=0), B, None, 1, "1f3:256:flat:2:2:0"),
    "flat-pool-shifted": (fwd(2, 8, 32, 48, 0, 48, pool=True, pool_shifted=1), B, None, 1, "1f3:256:flat:2:2:0"),
    "flat-pool-4x4": (fwd(48, 4, 4, 48, 0, 48, pool=True, pool_shifted=1), B, None, 1, "1f3:256:flat:2:3:0"),
    "flat-m40": (fwd(4, 8, 8, 64, 0, 40), P, (3, 3, 2, 64), 1, "1f4:256:flat:2:1:0"),                            # last block 8 channels: lcpp = 0
    "flat-fwd": (fwd(8, 8, 8, 96, 0, 96), B, None, 1, "1f3:256:flat:3:2:0"),
    "flat-fwd-up": (fwd(2, 16, 16, 96, 48, 96, up0=True), B, None, 1, "1f3:256:flat:3:2:0"),
    "flat-fwd-up-4x4": (fwd(32, 4, 4, 48, 48, 96, up0=True), B, None, 1, "1f3:256:flat:3:2:0"),
    "flat-t": (dgrad(128, 2, 2, 48, 0, 48), B, None, 1, "1t3:256:flat:2:2:0"),
    "flat-t-add": (dgrad(2, 16, 16, 48, 0, 48, add=True), B, None, 1, "1t3:256:flat:2:2:0"),
    "flat-t-mask": (dgrad(8, 8, 8, 96, 0, 96, mask=True), B, None, 1, "1t3:256:flat:3:2:0"),
}

# ---- the remaining instantiations: one chunk of KS x 16 channels, 272 tiles of 16 pixels, blocks of 96 + 64 and of 96 + 32 channels ------------
for _bf in "ft":
    for _ks in (1, 2, 3, 4):
        _mk = fwd if _bf == "f" else dgrad
        _kw = dict(mask=True, add=True) if _bf == "t" else {}
        CASES["fill-%s%d-rem2" % (_bf, _ks)] = (_mk(1, 68, 62, 16 * _ks, 0, 160, **_kw), B if _ks & 1 else P, (2, 2, 0, 16 * _ks), 1,
                                               "3%s%d:256:pipe:1:272:0+2%s%d:256:pipe:1:272:96" % (_bf, _ks, _bf, _ks))
        CASES["fill-%s%d-rem1" % (_bf, _ks)] = (_mk(1, 66, 64, 16 * _ks, 0, 120, **_kw), P if _ks & 1 else B, (2, 2, 0, 16 * _ks), 1,
                                               "3%s%d:256:pipe:1:272:0+1%s%d:256:allw:1:272:96" % (_bf, _ks, _bf, _ks))

# ---- 512 threads (8 waves, tiles of 257..512 pixels): no plan launches these; a parametrization of their own on the GPU ---------------------
WIDE = {
    "wide-pipe3-f4": (fwd(65, 17, 33, 64, 0, 96), B, (5, 4, 0, 64), 1, "3f4:512:pipe:1:260:0"),
    "wide-pipe2-dst32": (fwd(2, 20, 40, 32, 0, 40, dst32=True), P, (5, 4, 0, 32), 1, "2f2:512:pipe:1:8:0"),      # dst32: never 32-channel blocks
    "wide-allw-nblk2": (fwd(2, 32, 32, 64, 0, 64), B, (5, 4, 0, 64), 1, "1f4:512:allw:2:4:0"),
    "wide-allw-nblk3": (fwd(1, 96, 90, 64, 0, 96), B, (5, 4, 0, 64), 1, "1f4:512:allw:3:18:0"),
    "wide-async3": (fwd(2, 20, 40, 96, 0, 96), O, (5, 4, 0, 32), 1, "1f2:512:async:3:8:0"),
    "wide-async2-t": (dgrad(1, 48, 40, 96, 0, 160, mask=True), O, (4, 4, 1, 48), 1, "1t3:512:async:5:9:0"),
}
for _bf in "ft":
    for _ks in (1, 2, 3, 4):
        _mk = fwd if _bf == "f" else dgrad
        _kw = dict(mask=True, add=True) if _bf == "t" and _ks & 1 else {}
        WIDE["wide-fill-%s%d-rem2" % (_bf, _ks)] = (_mk(129, 5, 33, 16 * _ks, 0, 160, **_kw), B if _ks & 1 else P, (5, 4, 0, 16 * _ks), 1,
                                                   "3%s%d:512:pipe:1:258:0+2%s%d:512:pipe:1:258:96" % (_bf, _ks, _bf, _ks))
        WIDE["wide-fill-%s%d-rem1" % (_bf, _ks)] = (_mk(173, 3, 33, 16 * _ks, 0, 128, **_kw), P if _ks & 1 else B, (4, 4, 1, 16 * _ks), 1,
                                                   "3%s%d:512:pipe:1:%d:0+1%s%d:512:allw:1:%d:96" % (_bf, _ks, 87 * 3, _bf, _ks, 87 * 3))
ALL = dict(CASES, **WIDE)

# every instantiation the library builds (csrc/conv_mfma.hip::conv_launch_ks): (MT, BF, KS, threads)
INSTANTIATIONS = {(mt, bf, ks, th) for mt in (1, 2, 3) for bf in (0, 1) for ks in (1, 2, 3, 4) for th in (256, 512)} | {(1, 0, 6, 256), (1, 1, 6, 256)}


def _taps(name):
    from ssdn.hip import graph
    return {B: graph.TAPS_BLIND, P: graph.TAPS_PLAIN, O: graph.TAPS_1x1}[name]


def make_case(name, ints, device):
    kw, taps, tile, _, _ = ALL[name]
    if ints and kw.get("pool"):
        kw = dict(kw, act=True)           # the fused pool needs the activation: ints_expected follows the fp32 chain behind the exact sum
    return Case(taps=_taps(taps), tile=tile, ints=ints, device=device, seed=list(ALL).index(name), **kw)


def regime(launches):
    """ssdn_conv_variant's answer in the table's notation"""
    return "+".join("%d%s%d:%d:%s:%d:%d:%d" % (v["MT"], "ft"[v["BF"]], v["KS"], v["threads"], PATHS[v["path"]], v["nblk"], v["tiles"], v["m_base"])
                    for v in launches)


def parse(want):
    """the table's notation -> [(MT, BF, KS, threads, path, nblk, tiles, m_base)]"""
    out = []
    for part in want.split("+"):
        inst, th, path, nblk, tiles, mb = part.split(":")
        out.append((int(inst[0]), "ft".index(inst[1]), int(inst[2:]), int(th), PATHS.index(path), int(nblk), int(tiles), int(mb)))
    return out


def nsteps(name):
    kw, taps, tile, _, want = ALL[name]
    return len(_taps(taps)) * (kw["c0"] + kw["c1"]) // (16 * parse(want)[0][2])


def launch_class(a, v):
    """(path, MT, BF, KS, nblk > 1, ragged, m_base > 0, dst32, pool, upsum, mask, add, up0, c1 > 0) of one k_conv launch of arguments a"""
    ragged = bool(a.H % (1 << a.lth) or a.W % (1 << a.ltw) or a.N % (1 << a.ltn))
    return (v["path"], v["MT"], v["BF"], v["KS"], v["nblk"] > 1, ragged, v["m_base"] > 0, bool(a.dst32), bool(a.pool.p), bool(a.upsum.p),
            bool(a.mask.p), bool(a.add.p), bool(a.up0), a.c1 > 0)


@pytest.fixture(autouse=True)
def mode_reset():
    yield
    from ssdn.hip import lib as L
    L.load().ssdn_conv_set_mode(1)


def _table_classes():
    from ssdn.hip import lib as L
    lib = L.load()
    out = set()
    for name in ALL:
        L.check(lib.ssdn_conv_set_mode(ALL[name][3]))
        case = make_case(name, ints=False, device=False)
        out |= {launch_class(case.a, v) for v in case.variant()}
    lib.ssdn_conv_set_mode(1)
    return out


@pytest.mark.parametrize("name", list(ALL))
def test_case_reaches_its_regime_and_its_integer_reference_is_exact(name):
    from ssdn.hip import lib as L
    lib = L.load()
    kw, taps, tile, mode, want = ALL[name]
    L.check(lib.ssdn_conv_set_mode(mode))
    case = make_case(name, ints=True, device=False)
    ref = C.byref(case.a)
    assert lib.ssdn_conv_lds_bytes(ref) > 0, lib.ssdn_last_error()
    assert regime(case.variant()) == want
    if mode == 0:       # "k_conv always" only where the route would give the shape to another kernel
        L.check(lib.ssdn_conv_set_mode(1))
        assert case.variant() == [], "mode 1 already gives the case to k_conv"
        L.check(lib.ssdn_conv_set_mode(0))
    if kw.get("pool"):
        assert lib.ssdn_conv_fuses_pool(ref) == 1
    if kw.get("upsum_c"):
        assert lib.ssdn_conv_fuses_upsum(ref) == 1
    assert kw["N"] * kw["H"] * kw["W"] <= 85000 or name.startswith("eval-")
    # the reference is made of integers <= INT_LIMIT (ints_expected asserts it on the sums themselves), and where the weight rows have
    # enough entries for it, every (tap, channel) position of the weights is hit
    want_out = case.ints_expected()
    assert all(float(t[~t.isnan()].float().abs().max()) <= INT_LIMIT for t in want_out.values())
    if 32 * case.M >= 2 * len(case.taps) * case.Ktot:
        assert int(case.w_hits.min()) >= 1


def test_every_instantiation_is_reached():
    reached = {v[:4] for _, _, _, _, want in ALL.values() for v in parse(want)}
    assert reached == INSTANTIATIONS, "not reached: %s; not built: %s" % (sorted(INSTANTIATIONS - reached), sorted(reached - INSTANTIATIONS))
    assert len(INSTANTIATIONS) == 50
    assert {v[3] for c in WIDE.values() for v in parse(c[4])} == {512} and {v[3] for c in CASES.values() for v in parse(c[4])} == {256}
    assert {v[4] for _, _, _, _, want in ALL.values() for v in parse(want)} == {0, 1, 2, 3}


@pytest.mark.parametrize("path", ["pipe", "async"])
def test_step_counts_take_every_residue_mod_6(path):
    """the pipelined loop is unrolled six ways with five early exits, and the ASYNC tile buffers alternate by step parity"""
    res = {}
    for name, (_, _, _, _, want) in ALL.items():
        if parse(want)[0][4] == PATHS.index(path):
            res.setdefault(nsteps(name) % 6, []).append(name)
    assert sorted(res) == [0, 1, 2, 3, 4, 5], res


PLANS = [(3, 9, True, 32, 64, 64, True), (3, 9, True, 1, 512, 512, False), (3, 9, True, 1, 768, 768, False), (3, 3, False, 1, 352, 512, False),
         (3, 3, False, 1, 512, 352, False), (3, 3, False, 2, 96, 64, True)]


def test_plans_are_those_of_the_cdma_walk_and_a_non_square_training_plan():
    from test_cdma_walk_cpu import PLANS as CDMA_PLANS
    assert PLANS == CDMA_PLANS + [(3, 3, False, 2, 96, 64, True)]


@pytest.mark.parametrize("cin,cout,bs,Bn,H,W,train", PLANS)
def test_every_launch_class_of_the_plans_has_a_case(cin, cout, bs, Bn, H, W, train):
    from gen_golden_routes import plan_args
    from ssdn.hip import lib as L
    from ssdn.hip.graph import NetPlan
    from conv_case import VARIANT_FIELDS
    lib = L.load()
    table = _table_classes()
    plan = NetPlan("m/", cin, cout, bs, Bn, H, W, cus=256, dev_cus=256, train=train)
    launches = 0
    for op in plan.fwd + plan.bwd:
        if op.type != "conv":
            continue
        a = plan_args(plan, op.a)
        out = (C.c_int32 * 16)()
        rc = lib.ssdn_conv_variant(C.byref(a), out)
        assert rc >= 0, lib.ssdn_last_error()
        for i in range(rc):
            launches += 1
            v = dict(zip(VARIANT_FIELDS, out[8 * i:8 * i + 8]))
            assert launch_class(a, v) in table, "%s %s (%d, %d, %d): no case runs k_conv as this launch does: %s %s" % (
                op.a["layer"], op.a["role"], a.N, a.H, a.W, v, launch_class(a, v))
    assert launches >= 5          # (the 768x768 evaluation plan has the fewest: its larger stages run k_cdma)


def test_variant_query_answers():
    """invalid arguments: < 0 and a message; a launch another kernel serves: 0; the same launch under "k_conv always": its k_conv launches"""
    from ssdn.hip import graph, lib as L
    lib = L.load()
    out = (C.c_int32 * 16)()
    bad = L.ConvArgs()
    assert lib.ssdn_conv_variant(C.byref(bad), out) < 0 and b"ntaps" in lib.ssdn_last_error()
    assert lib.ssdn_conv_variant(None, out) < 0 and lib.ssdn_conv_variant(C.byref(bad), None) < 0
    # a tiling the launch would refuse: kc = 96 in blocks of 96 channels; a fused max-pool off the flat path
    big = Case(taps=graph.TAPS_BLIND, tile=(2, 2, 0, 96), device=False, **fwd(1, 68, 64, 96, 0, 96))
    assert lib.ssdn_conv_variant(C.byref(big.a), out) < 0 and b"kc" in lib.ssdn_last_error()
    pool = Case(taps=graph.TAPS_BLIND, tile=(4, 4, 0, 48), device=False, **fwd(2, 32, 32, 48, 0, 48, pool=True))
    assert lib.ssdn_conv_variant(C.byref(pool.a), out) < 0 and b"max-pool" in lib.ssdn_last_error()
    others = {
        "k_cdma": (1, -1, Case(taps=graph.TAPS_BLIND, cm=True, device=False, **fwd(128, 64, 64, 48, 0, 96))),
        "k_gdma": (1, -1, Case(taps=graph.TAPS_1x1, device=False, **fwd(1, 16, 16, 96, 0, 96))),
        "k_conv_thin": (1, -1, Case(taps=graph.TAPS_PLAIN, device=False, kreal=3, **fwd(2, 16, 64, 16, 0, 48))),
        "k_conv16": (1, 3, Case(taps=graph.TAPS_BLIND, device=False, **fwd(3, 16, 16, 96, 0, 96))),
    }
    try:
        for kernel, (mode, roles, case) in others.items():
            L.check(lib.ssdn_conv_set_mode(mode))
            L.check(lib.ssdn_conv_set_conv16(roles))
            assert case.variant() == [], "%s: the query counts k_conv launches" % kernel
            L.check(lib.ssdn_conv_set_mode(0))
            assert len(case.variant()) >= 1, kernel
    finally:
        lib.ssdn_conv_set_conv16(-1)
