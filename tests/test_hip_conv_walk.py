"""GPU: k_conv (csrc/conv_mfma.hip) per launch -- its four K loops, ragged tiles, fused epilogues and every instantiation.

k_conv<MT, BF, KS, threads> is the kernel SSDN_OP_CONV falls back to and the one k_conv16 is measured against.  State lives across its
pipeline steps (three weight register sets, two LDS weight buffers by step parity, a six-way unrolled loop with five early exits, a
per-workgroup tap rotation, the ASYNC tile buffers), its grid is rounded up to 8 tiles per channel block, and its three epilogues clip at the
image edge each in their own way; the per-op tests run of it what the planner emits at fixture sizes.  The table of
tests/test_conv_walk_cpu.py holds one direct SSDN_OP_CONV launch per regime, launch class of the full-size plans and instantiation (the id
names the regime); each runs twice:
  * ints: integer operands whose sums do not depend on the accumulation order (followed, where the launch has the activation or the fp32
    output, through the kernel's fixed fp32 chain: conv_case.Case.ints_expected) -- bit equality over the whole NaN-poisoned wide tensors,
    the fused max-pool's and up-sum's included, and over the fp32 buffer between its guards: a tile, row, channel block or image that was
    never stored is a NaN left, one stored twice from the wrong block a wrong integer;
  * rand: the random operands of conv_case.Case within the bounds of test_every_op_teacher_forced (conv_case._check_ref, _check_dst32); the
    fused max-pool output is exactly the pool of the stored output.
What ssdn_conv_variant answers on the device is appended to conv_walk.txt in the suite's output directory; where the device has the 256
compute units the table was computed for, it must be the table's regime, and on any device the launch counters must count the k_conv
launches the query promised and no launch of k_gdma or k_cdma.  The reference of the cases with more than 100 000 pixels is evaluated, by
the same formula in float64, on the device.

The 512-thread instantiations (8 waves, tiles of 257..512 pixels), which no plan launches, are a parametrization of their own."""
import ctypes as C
import os

import pytest
import torch

from conv_case import _check_dst32, _check_ref, check_ints, check_pool
from test_hip_ops import OUTDIR
from test_conv_walk_cpu import ALL, CASES, WIDE, make_case, nsteps, regime

pytestmark = pytest.mark.gpu

REPORT = os.path.join(OUTDIR, "conv_walk.txt")
KINDS = (0, 1, 2, 4, 5, 6)            # launch counters: k_conv<3 / 2 / 1>, k_gdma, k_cdma<3>, k_cdma<2 / 1>


def _lib():
    from ssdn.hip import lib as L
    return L, L.load()


@pytest.fixture(scope="module", autouse=True)
def report():
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "w") as f:
        f.write("# case operands: steps (taps x chunks), what ssdn_conv_variant answered on the device (compute units: %d) as\n"
                "# <MT><f|t><KS>:<threads>:<path>:<nblk>:<tiles>:<m_base> per launch\n" % _lib()[1].ssdn_device_cus())
    yield


@pytest.fixture(autouse=True)
def walk_reset():
    L, lib = _lib()
    L.check(lib.ssdn_conv_set_mode(1))
    for k in KINDS:
        L.check(lib.ssdn_profile_enable(k, 4))
        L.check(lib.ssdn_profile_set_stride(k, 1))
    _counts(lib)
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


def _walk(name, operands):
    L, lib = _lib()
    kw, taps, tile, mode, want = ALL[name]
    L.check(lib.ssdn_conv_set_mode(mode))
    case = make_case(name, ints=operands == "ints", device=True)
    launches = case.variant()
    with open(REPORT, "a") as f:
        f.write("%s %s: steps %d, %s\n" % (name, operands, nsteps(name), regime(launches)))
    assert launches, "ssdn_conv_variant: k_conv does not serve the launch"
    if lib.ssdn_device_cus() == 256:
        assert regime(launches) == want
    _counts(lib)
    got = case.launch()
    n = _counts(lib)
    promised = {k: sum(1 for v in launches if 3 - v["MT"] == k) for k in KINDS}
    assert n == promised, "launch counters %s: the query promised %s" % (n, promised)
    dev = torch.device("cuda:0") if kw["N"] * kw["H"] * kw["W"] > 100000 else None
    if operands == "ints":
        check_ints(case, got, dev)
    elif "dst32" in got:
        _check_dst32(case, got, dev)
    else:
        _check_ref(case, got, dev=dev)
        if case.pool:
            check_pool(case, got)
    assert case.inputs_intact(), "an input tensor was written"


@pytest.mark.parametrize("operands", ["ints", "rand"])
@pytest.mark.parametrize("name", list(CASES))
def test_conv_walk(name, operands):
    _walk(name, operands)


@pytest.mark.parametrize("operands", ["ints", "rand"])
@pytest.mark.parametrize("name", list(WIDE))
def test_conv_walk_wide(name, operands):
    _walk(name, operands)
