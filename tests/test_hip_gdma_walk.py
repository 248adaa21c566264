"""GPU: k_gdma's tile walk and epilogues (csrc/gemm_dma.hip) per launch -- ragged walks, ring phases, the fused un-rotation, fused pairs.

The 1x1 layers of the posterior head run on a persistent kernel: grid = min(tiles, compute units) workgroups walk 256-pixel tiles, and the
two operand rings (depth 3) run on as one chunk stream across a workgroup's tiles.  The table of tests/test_gdma_walk_cpu.py holds one
direct SSDN_OP_CONV launch per regime of that walk and kernel instantiation (the id names regime, variant and instantiation: tile width,
f / t for forward fp16 / data gradient bf16, EPI); each runs twice:
  * ints: integer operands whose sums do not depend on the accumulation order, followed through the epilogue's fixed fp32 chain
    (conv_case.Case._ints_chain) -- bit equality over the whole NaN-poisoned wide tensors: a tile, pixel, channel block or row that was
    never stored is a NaN left, one stored twice from the wrong stage a wrong integer;
  * rand: the random operands of conv_case.Case within the bounds of test_every_op_teacher_forced (conv_case._check_ref; the second
    layer of a fused pair: the forward bound on fp32, conv_case._check_next32).
The launch counters must say exactly one SSDN_PROF_GEMM launch and nothing else -- a fused pair is one launch for two records, and both
its outputs must be bit-identical to the two separate launches under ssdn_conv_set_chain(0).  Where the device has the 256 compute units
the regimes are named for, the walk must be the one named.  The reference of the cases with more than 100 000 pixels is evaluated, by the
same formula in float64, on the device.

What ran is appended to gdma_walk.txt in the suite's output directory."""
import ctypes as C
import os

import pytest
import torch

from conv_case import _check_next32, _check_ref, _same, check_ints, check_signs
from test_hip_ops import OUTDIR
from test_gdma_walk_cpu import CASES, IDS, REGIMES, TILE, VARIANTS, make_case, walk

pytestmark = pytest.mark.gpu

REPORT = os.path.join(OUTDIR, "gdma_walk.txt")


def _lib():
    from ssdn.hip import lib as L
    return L, L.load()


@pytest.fixture(scope="module", autouse=True)
def report():
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "w") as f:
        f.write("# case operands: launches counted, the walk of its tiles on this device (compute units: %d)\n" % _lib()[1].ssdn_device_cus())
    yield


@pytest.fixture(autouse=True)
def walk_reset():
    L, lib = _lib()
    for k in L.PROF.values():
        L.check(lib.ssdn_profile_enable(k, 4))
        L.check(lib.ssdn_profile_set_stride(k, 1))
    yield
    lib.ssdn_conv_set_chain(1)
    lib.ssdn_conv_set_mode(1)
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


@pytest.mark.parametrize("operands", ["ints", "rand"])
@pytest.mark.parametrize("regime,variant", CASES, ids=IDS)
def test_gdma_walk(regime, variant, operands):
    L, lib = _lib()
    (N, H, W), want = REGIMES[regime]
    case = make_case(regime, variant, ints=operands == "ints", device=True)
    cus = lib.ssdn_device_cus()
    w = walk(N * H * W // TILE, cus)
    if cus == 256:
        assert w == want, "the case does not walk as its regime says: %s" % w
    _counts(lib)
    got = case.launch()
    n = _counts(lib)
    with open(REPORT, "a") as f:
        f.write("%s-%s-%s %s: %s %s\n" % (regime, variant, VARIANTS[variant][1], operands, {k: v for k, v in n.items() if v}, w))
    assert n == dict(dict.fromkeys(L.PROF, 0), gemm=1), "launch counters %s: not the one k_gdma launch the case is there for" % n
    dev = torch.device("cuda:0") if N * H * W > 100000 else None
    if operands == "ints":
        check_ints(case, got, dev)
    else:
        _check_ref(case, got, dev=dev)
        if case.next is not None:
            _check_next32(case, got, dev)
    check_signs(case, got)
    assert case.inputs_intact(), "an input tensor was written"
    if case.next is not None:
        # the two records as two launches: k_gdma for the first, the general kernel for the narrow layer -- the same bits
        L.check(lib.ssdn_conv_set_chain(0))
        apart = case.launch()
        n = _counts(lib)
        assert n["gemm"] == 1 and sum(n.values()) == 2, "launch counters %s: not two separate launches" % n
        _same(got, apart, "fused pair against the two separate launches")
