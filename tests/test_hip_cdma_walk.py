"""GPU: k_cdma's tile walk (csrc/conv_dma.hip) per launch -- long strips, segments, second work items.

A workgroup of the persistent kernel walks work items of `tps` consecutive 16x16 tiles and, out of tiles, takes item + stride.  The tile
and weight buffer parities, the next-tile prefetch, the per-XCD item ranges, the row arithmetic of a segment and the reciprocal of the
tile-column count all live across tiles and items; the per-op tests of tests/test_hip_ops.py run them with one item per workgroup and at
most three tiles per item.  The table of tests/test_cdma_walk_cpu.py holds one direct SSDN_OP_CONV launch per regime and kernel
instantiation the full-size plans use (the id names regime, operands and instantiation (MT, BF, EPI, KIND)); each runs twice:
  * ints: integer operands whose result does not depend on the accumulation order -- bit equality with the float64 reference cast to
    the output type, over the whole NaN-poisoned wide tensors (a tile, row, channel or image that was never stored is a NaN left);
  * rand: the random operands of conv_case.Case within the bounds of test_every_op_teacher_forced (conv_case._check_ref).
That k_cdma served the launch is read from the launch counters and from ssdn_conv_dma_split on the device, which must also report the
regime the case is there for (where the device has the 256 compute units the shapes were computed for).  The reference of the cases with
more than 100 000 pixels is evaluated, by the same formula in float64, on the device.

What the device answered per case is appended to cdma_walk.txt in the suite's output directory."""
import ctypes as C
import os

import pytest
import torch

from conv_case import _check_ref, check_ints, check_signs
from test_hip_ops import OUTDIR
from test_cdma_walk_cpu import CASES, IDS, REGIMES, VARIANTS, make_case, regime_reached

pytestmark = pytest.mark.gpu

REPORT = os.path.join(OUTDIR, "cdma_walk.txt")
KINDS = (0, 1, 2, 4, 5, 6)            # launch counters: k_conv<3 / 2 / 1>, k_gdma, k_cdma<3>, k_cdma<2 / 1>


def _lib():
    from ssdn.hip import lib as L
    return L, L.load()


@pytest.fixture(scope="module", autouse=True)
def report():
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "w") as f:
        f.write("# case: what ssdn_conv_dma_split answered on the device (compute units: %d)\n" % _lib()[1].ssdn_device_cus())
    yield


@pytest.fixture(autouse=True)
def walk_reset():
    L, lib = _lib()
    for k in KINDS:
        L.check(lib.ssdn_profile_enable(k, 4))
    yield
    lib.ssdn_conv_set_mode(1)
    for k in KINDS:
        lib.ssdn_profile_enable(k, 0)


def _counts(lib):
    L = _lib()[0]
    out = {}
    for k in KINDS:
        ms, n, fl, by = C.c_double(), C.c_longlong(), C.c_double(), C.c_double()
        L.check(lib.ssdn_profile_read(k, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)))
        out[k] = n.value
    return out


@pytest.mark.parametrize("operands", ["ints", "rand"])
@pytest.mark.parametrize("regime,variant", CASES, ids=IDS)
def test_cdma_walk(regime, variant, operands):
    L, lib = _lib()
    (N, H, W), mode, want = REGIMES[regime]
    L.check(lib.ssdn_conv_set_mode(mode))
    case = make_case(regime, variant, ints=operands == "ints", device=True)
    served, split = case.split()
    with open(REPORT, "a") as f:
        f.write("%s-%s-%s %s: k_cdma %d %s\n" % (regime, variant, VARIANTS[variant][2], operands, served, split))
    assert served == 1, "ssdn_conv_dma_split: k_cdma does not serve the launch"
    if lib.ssdn_device_cus() == 256:
        assert regime_reached(split, want) is None, regime_reached(split, want)
    _counts(lib)
    got = case.launch()
    n = _counts(lib)
    mt3, mt21 = VARIANTS[variant][3]
    assert n == {0: 0, 1: 0, 2: 0, 4: 0, 5: mt3, 6: mt21}, "launch counters %s: not the k_cdma launches the case is there for" % n
    dev = torch.device("cuda:0") if N * H * W > 100000 else None
    if operands == "ints":
        check_ints(case, got, dev)
    else:
        _check_ref(case, got, dev=dev)
    check_signs(case, got)
    assert case.inputs_intact(), "an input tensor was written"
