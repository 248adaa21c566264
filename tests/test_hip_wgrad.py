"""GPU: SSDN_OP_WGRAD per launch -- every row of the case table of tests/wgrad_case.py (one per kernel variant: the three static schedules,
the two-load variant, both BOTH forms, the synchronous mode, column groups, mblocks, up0, several images per tile, k_wgrad_thin, an empty
share) under the four operand generators, against the header's formula in float64:

  * the sum over the slabs, taken in float64 on the host before any reduction, on the real region (rows m < M, columns k < the real
    channels of the tap; padding holds unspecified values): finite, and bit-equal to the expectation for ints, round and probe, within the
    derived bound for rand;
  * through SSDN_OP_WREDUCE with inv_scale = 1.0 into a NaN-filled layer-shaped gradient: the block holds the expectation in OIHW order
    (tap-block order for the 1x1 layers over channel blocks), every element outside it is still NaN;
  * the inputs' guard channels and guard strips are still NaN;
  * one merged launch of all rows that have an instance in it (k_wgrad_mega; k_wgrad_multi for the mergeable rows): every op still meets
    its expectation -- the call sites of the thin body that only the merged kernel has included;
  * a second run gives the same slab bits.
tests/test_wgrad_case_cpu.py holds the table to its classes and to the BASELINE plans.  The variant the library reports for every row and
the rand generator's max err / bound are written to wgrad_cases.txt under OUTDIR."""
import ctypes as C
import os

import pytest
import torch

from test_hip_ops import OUTDIR
from wgrad_case import GENS, NAMES, make

pytestmark = pytest.mark.gpu


def _lib():
    from ssdn.hip import lib as L
    return L, L.load()


@pytest.fixture(scope="module")
def report():
    os.makedirs(OUTDIR, exist_ok=True)
    path = os.path.join(OUTDIR, "wgrad_cases.txt")
    with open(path, "w") as f:
        f.write("# row generator: instance in the chip-wide launch, out9 = (thin, MT, CPW, NL, BOTH, PS, KS, RWX, RWD); differing elements / max err / bound\n")

    def line(text):
        with open(path, "a") as f:
            f.write(text + "\n")
    return line


@pytest.fixture
def launch_counters():
    """SSDN_PROF_WGRAD / SSDN_PROF_WGRAD_SIDE count every launch while the test runs -> read() = (launches, side-lane launches)"""
    L, lib = _lib()
    kinds = (L.PROF["wgrad"], L.PROF["wgrad_side"])
    for k in kinds:
        L.check(lib.ssdn_profile_enable(k, 16))
        L.check(lib.ssdn_profile_set_stride(k, 1))

    def read():
        out = []
        for k in kinds:
            ms, n, fl, by = C.c_double(), C.c_longlong(), C.c_double(), C.c_double()
            L.check(lib.ssdn_profile_read(k, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)))
            out.append(n.value)
        return tuple(out)
    yield read
    for k in kinds:
        lib.ssdn_profile_enable(k, 0)


@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("name", NAMES)
def test_launch_alone(name, gen, report):
    case = make(name, gen)
    inst, out9 = case.variant()
    ratio = case.check_all()
    report("%-16s %-5s: instance %3d, out9 %s; %s" % (name, gen, inst, out9, "max err / bound %.4f" % ratio if gen == "rand" else "0 elements differ"))


@pytest.mark.parametrize("name", NAMES)
def test_second_run_gives_the_same_slab_bits(name):
    """the real region (padded rows and columns hold whatever the LDS held)"""
    case = make(name, "rand")
    first, second = case.real(*case.launch()), case.real(*case.launch())
    for a, b in zip(first, second):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("name,gen", [("st8", "probe"), ("ragged", "ints"), ("thin_k3", "probe")])
def test_the_checks_notice_a_wrong_launch(name, gen):
    """the taps mirrored in x -- the same halo, another pairing of taps and pixels -- miss the expectation; slabs nobody wrote do too"""
    case = make(name, gen)
    case.poison()
    with pytest.raises(AssertionError, match="never stored"):
        case.check_slabs(*case.slabs())
    for t in range(case.ntaps):
        case.a.dx[t] = -case.a.dx[t]
    with pytest.raises(AssertionError, match="elements differ"):
        case.check_slabs(*case.launch())


def _merged(gen, mega, launch_counters):
    """all rows the merged kernel has an instance for as ONE op list -> the cases, after the run (slabs not yet reduced)"""
    from ssdn.hip.engine import OpList, current_stream
    L, lib = _lib()
    cus = lib.ssdn_device_cus()
    cases = []
    for name in NAMES:
        case = make(name, gen)
        inst, out9 = case.variant()
        if mega:
            # the planner's cost model in outline: K-steps of the longest share x (660 + 90 column tiles per wave) cycles
            case.a.mega = cus
            case.a.cost = float(-(-case.ntiles // case.nslabs) * (case.TW * case.TH * case.TN // 16) * (660 + 90 * out9[2]))
            if inst < 0:
                continue
            assert lib.ssdn_wgrad_mega_ok(C.byref(case.a)) == 1
        elif not lib.ssdn_wgrad_mergeable(C.byref(case.a)):
            continue
        cases.append((name, case))
    assert len(cases) >= 12, "the table must exercise the merged launch (%d rows with an instance in it)" % len(cases)
    for _, case in cases:
        case.poison()
    launch_counters()
    OpList([("wgrad", case.a) for _, case in cases]).run(current_stream())
    torch.cuda.synchronize()
    # k_wgrad_mega takes up to 64 ops, k_wgrad_multi up to 32: the executor cuts a longer run
    cap = 64 if mega else 32
    assert launch_counters() == (-(-len(cases) // cap), 0), "the run was not merged"
    return cases


def _check_merged(cases):
    for name, case in cases:
        try:
            case.check_slabs(*case.slabs())
            case.check_reduced(*case.reduce())
            assert case.inputs_intact()
        except AssertionError as e:
            raise AssertionError("%s inside the merged launch: %s" % (name, e))


@pytest.mark.parametrize("gen", GENS)
def test_chip_wide_launch_of_the_table(gen, launch_counters):
    """k_wgrad_mega: every block runs the code of its op's own launch; the thin rows run wgrad_thin_body from here"""
    cases = _merged(gen, True, launch_counters)
    names = [n for n, _ in cases]
    assert {"thin_k1", "thin_k2", "thin_k3", "thin_src1", "thin_empty", "st8", "st8_nl2", "st4b_mb4", "ragged", "tn4_sync_g2"} <= set(names), names
    _check_merged(cases)


@pytest.mark.parametrize("gen", GENS)
def test_small_layer_launch_of_the_table(gen, launch_counters):
    """k_wgrad_multi (mega = 0): the mergeable rows as one launch, each on the run-time-staged instance of its (MT, CPW, BOTH)"""
    _check_merged(_merged(gen, False, launch_counters))
