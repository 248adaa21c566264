"""GPU: the launch follows the queries.  One small SSDN_OP_CONV per kernel that serves the op (csrc/conv_mfma.hip::conv_route): what the
host-side queries say about the arguments -- tests/test_conv_route_cpu.py pins their answers -- is turned into the launches the library's
in-stream profiler must then count, kind by kind, and the output must be the float64 convolution of the same operands within the bounds of
tests/test_hip_ops.py::test_every_op_teacher_forced (conv_case._check_ref).  Only valid launches are made."""
import ctypes as C

import pytest

from conv_case import Case, _check_dst32, _check_ref

pytestmark = pytest.mark.gpu


def _lib():
    from ssdn.hip import lib as L
    return L, L.load()


def _taps(name):
    from ssdn.hip import graph
    return {"blind": graph.TAPS_BLIND, "plain": graph.TAPS_PLAIN, "1x1": graph.TAPS_1x1}[name]


# name -> (the kernel the case is there for, ssdn_conv_set_mode, ssdn_conv_set_conv16, taps, Case arguments)
CASES = {
    "cdma_96": ("k_cdma", 2, -1, "blind", dict(role="fwd", N=1, c0=96, c1=0, up0=False, M=96, cm=True)),       # one 16x16 image: one tile
    "cdma_160": ("k_cdma", 2, -1, "blind", dict(role="dgrad", N=1, c0=96, c1=0, up0=False, M=160, cm=True)),   # blocks of 96 + 64 channels
    "conv16": ("k_conv16", 1, 3, "blind", dict(role="fwd", N=3, c0=96, c1=0, up0=False, M=96)),
    "gdma_96": ("k_gdma", 1, -1, "1x1", dict(role="fwd", N=1, c0=96, c1=0, up0=False, M=96)),                  # 256 pixels: one tile
    "gdma_384": ("k_gdma", 1, -1, "1x1", dict(role="fwd", N=1, c0=96, c1=0, up0=False, M=384)),
    "thin": ("k_conv_thin", 1, -1, "plain", dict(role="fwd", N=2, c0=16, c1=0, up0=False, M=48, H=16, W=64, kreal=3)),
    "conv_mt1_flat": ("k_conv", 1, -1, "blind", dict(role="fwd", N=4, c0=48, c1=0, up0=False, M=64, H=8, W=8)),    # four whole images per tile
    "conv_mt3_rem": ("k_conv", 1, -1, "plain", dict(role="fwd", N=3, c0=96, c1=0, up0=False, M=100, dst32=True)),  # blocks of 96 + 32 channels
}


@pytest.fixture(autouse=True)
def route_reset():
    L, lib = _lib()
    for k in L.PROF.values():
        L.check(lib.ssdn_profile_enable(k, 4))
        L.check(lib.ssdn_profile_set_stride(k, 1))
    yield
    lib.ssdn_conv_set_mode(1)
    lib.ssdn_conv_set_conv16(-1)
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


def predicted(case, mode):
    """(kernel, launches per profiler kind) the host-side queries promise for the arguments under the settings in force"""
    L, lib = _lib()
    a, ref = case.a, C.byref(case.a)
    n = dict.fromkeys(L.PROF, 0)
    lds = lib.ssdn_conv_lds_bytes(ref)
    assert lds > 0, lib.ssdn_last_error()
    served, split = case.split()
    if served:
        n["cdma_mt3"] = min(split["mt_blocks"], a.Mpad // 96)            # blocks of 96 output channels, then one of 64 or 32
        n["cdma_mt21"] = split["mt_blocks"] - n["cdma_mt3"]
        return "k_cdma", n
    if case.eligible():
        n["conv_mt1"] = 1                                               # (k_conv16 counts as the launches it replaces)
        return "k_conv16", n
    L.check(lib.ssdn_conv_set_mode(0))                                  # "k_conv always": the LDS size k_conv has for the launch
    lds_k_conv = lib.ssdn_conv_lds_bytes(ref)
    L.check(lib.ssdn_conv_set_mode(mode))
    if lds != lds_k_conv:
        if a.ntaps == 1:
            n["gemm"] = 1
            return "k_gdma", n
        return "k_conv_thin", n                                         # (not profiled)
    if lib.ssdn_conv_fuses_pool(ref):                                   # the flat path: 32-channel blocks, all in one launch
        n["conv_mt1"] = 1
        return "k_conv", n
    assert a.dst32, "no query tells 32-channel from 96-channel blocks for this launch"      # (fp32 output: 96-channel blocks at any size)
    n["conv_mt3"] = 1 if a.Mpad >= 96 else 0
    rem = a.Mpad % 96 // 32
    if rem:
        n["conv_mt2" if rem == 2 else "conv_mt1"] += 1
    return "k_conv", n


@pytest.mark.parametrize("name", list(CASES))
def test_launch_follows_the_queries(name):
    L, lib = _lib()
    kernel, mode, roles, taps, kw = CASES[name]
    L.check(lib.ssdn_conv_set_mode(mode))
    L.check(lib.ssdn_conv_set_conv16(roles))
    case = Case(taps=_taps(taps), seed=len(name), **kw)
    said, want = predicted(case, mode)
    assert said == kernel, "the queries route the case to %s" % said
    _counts(lib)
    got = case.launch()
    n = _counts(lib)
    assert n == want, "launch counters %s: the queries promised %s" % (n, want)
    if "dst32" in got:
        _check_dst32(case, got)
    else:
        _check_ref(case, got)
    assert case.inputs_intact(), "an input tensor was written"
