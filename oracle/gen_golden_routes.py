#!/usr/bin/env python3
"""TEST INFRASTRUCTURE -- writes tests/golden/g_conv_routes.json: what the library's host-side queries answer for every SSDN_OP_CONV of a
grid of plans, as planned and with each fused output / sign-byte field toggled, under every setting of ssdn_conv_set_mode and
ssdn_conv_set_conv16.  tests/test_conv_route_cpu.py compares the library with this file, so a launch that changes its kernel, its LDS
size, its k_cdma work split or what it can fuse shows up as this file's diff: regenerate it ON PURPOSE only, and then from a build of
the commit whose routing is the reference (SSDN_HIP_LIB names another build of the library):

    SSDN_HIP_LIB=/path/to/libssdn_hip.so python oracle/gen_golden_routes.py      # host code only: no device is needed

The file holds the table of distinct outcomes and one index into it per case, in sweep order (cases()); the arguments are not stored:
the test rebuilds them from the plans.  Without a device the library answers for 256 compute units, and so do the plans.
"""
import ctypes as C
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "selfsupervised-denoising_amd"))

from ssdn.hip import lib as L  # noqa: E402
from ssdn.hip.graph import NetPlan  # noqa: E402

OUT = os.environ.get("SSDN_GOLDEN_OUT") or os.path.join(os.path.dirname(HERE), "tests", "golden")
NAME = "g_conv_routes.json"
DUMMY = 0x1000          # a non-null address: the queries read no memory

# (cin, cout, blindspot, B, H, W, train): the plan lists of tests/test_conv16_cpu.py and tests/test_cdma_walk_cpu.py
PLANS = [(3, 9, True, 32, 64, 64, True), (3, 9, True, 2, 64, 64, True), (3, 1, False, 32, 64, 64, True), (3, 3, False, 32, 64, 64, True),
         (3, 3, False, 300, 64, 64, True), (3, 3, False, 1, 256, 256, True), (3, 3, False, 2, 96, 64, True), (1, 2, True, 4, 32, 32, True),
         (3, 9, True, 1, 512, 512, False), (3, 9, True, 1, 768, 768, False), (3, 3, False, 1, 352, 512, False), (3, 3, False, 1, 512, 352, False)]
VIEW_FIELDS = ("pool", "upsum", "unrot", "urot")
SIGN_FIELDS = ("sign_out", "mask_sign", "upsum_mask_sign")
VARIANTS = ("planned",) + VIEW_FIELDS + SIGN_FIELDS + ("no_wc",)
# (ssdn_conv_set_mode, ssdn_conv_set_conv16); -1: the default roles
SETTINGS = [(0, -1), (2, -1), (1, 0), (1, 1), (1, 2), (1, 3)]
QUERIES = ("ssdn_conv_fuses_pool", "ssdn_conv_fuses_upsum", "ssdn_conv_fuses_unrot", "ssdn_conv_fuses_urot", "ssdn_conv_signs",
           "ssdn_conv16_eligible")
# an outcome: [ssdn_conv_lds_bytes, the six QUERIES, the return value of ssdn_conv_dma_split, its out8]
LDS, FIRST_QUERY, SPLIT_RC = 0, 1, 7


def make_plan(cin, cout, bs, B, H, W, train):
    return NetPlan("m/", cin, cout, bs, B, H, W, cus=256, dev_cus=256, train=train)


def plan_args(plan, a):
    """ssdn_conv_args of a planned op without a device: dummy addresses, the plan's own strides, the chunk-major weight copy where the
    plan has one"""
    def view(v):
        return L.View(DUMMY, plan.tensors[v.t].shape[-1], v.co) if v is not None else L.View(None, 0, 0)

    def ptr(field, name):
        if field == "wc" and plan.prefix + ("wfc/" if a["role"] == "fwd" else "wdc/") + name not in plan.tensors:
            return None
        return DUMMY
    return L.conv_args(a, view, ptr)


def variant_args(plan, a, variant):
    """the planned arguments with one field toggled: cleared if set, set to a dummy if clear (a view: the destination's)"""
    s = plan_args(plan, a)
    if variant in VIEW_FIELDS:
        setattr(s, variant, L.View(None, 0, 0) if getattr(s, variant).p else L.View(DUMMY, s.dst.cs, s.dst.co))
    elif variant in SIGN_FIELDS:
        setattr(s, variant, None if getattr(s, variant) else DUMMY)
    elif variant == "no_wc":
        s.wc = None
    return s


def cases():
    """(plan index, layer, role, variant, arguments) in sweep order; every one is asked under each of SETTINGS"""
    for p, shape in enumerate(PLANS):
        plan = make_plan(*shape)
        for op in plan.fwd + plan.bwd:
            if op.type == "conv":
                for v in VARIANTS:
                    yield p, op.a["layer"], op.a["role"], v, variant_args(plan, op.a, v)


def outcome(lib, s):
    out8 = (C.c_int32 * 8)()
    ref = C.byref(s)
    lds = lib.ssdn_conv_lds_bytes(ref)
    answers = [getattr(lib, q)(ref) for q in QUERIES]
    return [lds] + answers + [lib.ssdn_conv_dma_split(ref, out8)] + list(out8)


def sweep(lib):
    """[(plan index, layer, role, variant, mode, roles, arguments, outcome)] over cases() x SETTINGS; leaves the library at its defaults"""
    structs = list(cases())
    rows = [None] * (len(structs) * len(SETTINGS))
    try:
        for k, (mode, roles) in enumerate(SETTINGS):
            L.check(lib.ssdn_conv_set_mode(mode))
            L.check(lib.ssdn_conv_set_conv16(roles))
            for i, (p, layer, role, v, s) in enumerate(structs):
                rows[i * len(SETTINGS) + k] = (p, layer, role, v, mode, roles, s, outcome(lib, s))
    finally:
        lib.ssdn_conv_set_mode(1)
        lib.ssdn_conv_set_conv16(-1)
    return rows


def generate(lib) -> str:
    table, index = {}, []
    for row in sweep(lib):
        index.append(table.setdefault(tuple(row[-1]), len(table)))
    doc = dict(plans=[list(p) for p in PLANS], variants=list(VARIANTS), settings=[list(s) for s in SETTINGS],
               outcomes=[list(o) for o in table], cases=index)
    return json.dumps(doc, separators=(",", ":")) + "\n"


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    text = generate(L.load())
    with open(os.path.join(OUT, NAME), "w") as f:
        f.write(text)
    doc = json.loads(text)
    print("wrote %s from %s: %d cases, %d outcomes, %d bytes, sha256 %s" % (
        os.path.join(OUT, NAME), L.LIB_PATH, len(doc["cases"]), len(doc["outcomes"]), len(text), hashlib.sha256(text.encode()).hexdigest()))
