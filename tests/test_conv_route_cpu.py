"""CPU: which kernel serves an SSDN_OP_CONV, and everything the library says about that launch before it is made, is pinned.

csrc/conv_mfma.hip::conv_route decides the kernel of a launch once; ssdn_conv_lds_bytes, the four ssdn_conv_fuses_* queries,
ssdn_conv_signs, ssdn_conv16_eligible and ssdn_conv_dma_split are reads of that decision.  tests/golden/g_conv_routes.json
(oracle/gen_golden_routes.py) holds what they answered, the commit before the route existed, for every SSDN_OP_CONV of twelve plans -- as
planned, with each fused output and sign-byte field toggled and without the chunk-major weight copy -- under every setting of
ssdn_conv_set_mode and ssdn_conv_set_conv16.  Equality with the file, case by case, is "no launch changed its kernel, its LDS size, its
k_cdma work split or what it fuses".  The sweep must also reach what it is there for: all five kernels, and both answers of every query."""
import ctypes as C
import json
import os

import pytest

import gen_golden_routes as GEN
from conv_case import Case
from ssdn.hip import lib as L

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GEN.NAME)) as _f:
    GOLD = json.load(_f)


@pytest.fixture(autouse=True)
def settings_reset():
    yield
    L.load().ssdn_conv_set_mode(1)
    L.load().ssdn_conv_set_conv16(-1)


@pytest.fixture(scope="module")
def rows():
    return GEN.sweep(L.load())


def test_fixture_is_of_this_sweep(rows):
    assert GOLD["plans"] == [list(p) for p in GEN.PLANS] and GOLD["variants"] == list(GEN.VARIANTS)
    assert GOLD["settings"] == [list(s) for s in GEN.SETTINGS]
    assert len(GOLD["cases"]) == len(rows) >= 10000, "no case is skipped"
    assert len({tuple(o) for o in GOLD["outcomes"]}) == len(GOLD["outcomes"]) and max(GOLD["cases"]) == len(GOLD["outcomes"]) - 1


def test_every_query_answers_as_the_fixture(rows):
    bad = []
    for (p, layer, role, variant, mode, roles, _, got), k in zip(rows, GOLD["cases"]):
        if got != GOLD["outcomes"][k]:
            bad.append("plan %s %s %s, %s, mode %d roles %d: %s, the fixture has %s" % (
                GEN.PLANS[p], layer, role, variant, mode, roles, got, GOLD["outcomes"][k]))
    assert not bad, "%d of %d cases differ; the first: %s" % (len(bad), len(rows), "; ".join(bad[:5]))


def _kernels(rows):
    """which kernel each case of the sweep runs on, from the answers alone: k_cdma and k_conv16 say so themselves; a launch whose LDS
    size is not the one k_conv has for it (mode 0 is "k_conv always") went to k_gdma if it is a 1x1 layer and to k_conv_thin otherwise"""
    n = len(GEN.SETTINGS)
    assert GEN.SETTINGS[0][0] == 0
    out = []
    for i, (p, layer, role, variant, mode, roles, s, o) in enumerate(rows):
        k_conv_lds = rows[i - i % n][-1][GEN.LDS]
        if o[GEN.SPLIT_RC] == 1:
            k = "k_cdma"
        elif o[GEN.FIRST_QUERY + GEN.QUERIES.index("ssdn_conv16_eligible")]:
            k = "k_conv16"
        elif o[GEN.LDS] != k_conv_lds:
            k = "k_gdma" if s.ntaps == 1 else "k_conv_thin"
        else:
            k = "k_conv"
        out.append((mode, k))
    return out


def test_sweep_reaches_every_kernel_and_both_answers_of_every_query(rows):
    kernels = _kernels(rows)
    count = {k: sum(1 for m, kk in kernels if m == 1 and kk == k) for k in ("k_gdma", "k_conv_thin", "k_cdma", "k_conv16", "k_conv")}
    print(count)
    assert all(count.values()), count
    assert {k for m, k in kernels if m == 0} == {"k_conv"}
    assert not any(o[GEN.LDS] < 0 or o[GEN.SPLIT_RC] < 0 for *_, o in rows), "the plans hold valid launches only"
    for q, name in enumerate(GEN.QUERIES):
        assert {o[GEN.FIRST_QUERY + q] for *_, o in rows} == {0, 1}, name
    assert {o[GEN.SPLIT_RC] for *_, o in rows} == {0, 1}


def _error(lib):
    return lib.ssdn_last_error().decode()


def test_invalid_arguments_are_refused_with_their_message():
    lib = L.load()
    out8 = (C.c_int32 * 8)()
    bad = L.ConvArgs()                                   # ntaps = 0
    assert lib.ssdn_conv_lds_bytes(C.byref(bad)) < 0 and "ntaps" in _error(lib)
    assert lib.ssdn_conv_dma_split(C.byref(bad), out8) < 0 and "ntaps" in _error(lib)
    assert [getattr(lib, q)(C.byref(bad)) for q in GEN.QUERIES] == [0] * len(GEN.QUERIES)
    bad.ntaps = L.MAX_TAPS + 1
    assert lib.ssdn_conv_lds_bytes(C.byref(bad)) < 0 and "ntaps" in _error(lib)
    # kc = 96 exists for the launches that run as 32-channel blocks: at most one pixel tile per compute unit (256 without a device)
    from ssdn.hip import graph
    few = Case("fwd", 200, 96, 0, False, 96, graph.TAPS_BLIND, device=False)
    many = Case("fwd", 300, 96, 0, False, 96, graph.TAPS_BLIND, device=False)
    for case in (few, many):
        assert (case.a.ltw, case.a.lth, case.a.ltn) == (4, 4, 0)          # one 16x16 image per tile
        case.a.kc = 96
    for mode, roles in ((0, -1), (1, 0)):
        L.check(lib.ssdn_conv_set_mode(mode))
        L.check(lib.ssdn_conv_set_conv16(roles))
        assert lib.ssdn_conv_lds_bytes(C.byref(few.a)) > 0
        assert lib.ssdn_conv_lds_bytes(C.byref(many.a)) < 0 and "kc = 96" in _error(lib)
        assert lib.ssdn_conv_dma_split(C.byref(many.a), out8) == 0      # (the arguments themselves are valid)
    few.a.kc = 80
    assert lib.ssdn_conv_lds_bytes(C.byref(few.a)) < 0 and "kc must be" in _error(lib)
