"""CPU: which launches k_conv16 (csrc/conv16.hip) claims.  ssdn_conv16_eligible (host code) against the rule stated here in Python, over every
SSDN_OP_CONV of the planned forward and backward lists of the networks the BASELINE configurations train and evaluate: only the 96-channel
3x3 layers at 16x16 pixels with at most one image per CU may be claimed, and of those only the roles switched on."""
import ctypes as C

import pytest

from ssdn.hip import lib as L
from ssdn.hip.graph import NetPlan

DUMMY = 0x1000          # a non-null address: the predicate reads no memory

# (cin, cout, blindspot, B, H, W): the blind-spot RGB network at the training patch (configs 2, 3) and at batch 2; the sigma network (config 3);
# the plain networks (configs 4, 5) at the training patch, at a batch above one image per CU, at an evaluation size, and small inputs whose 16x16 stage is another decoder block
PLANS = [(3, 9, True, 32, 64, 64), (3, 9, True, 2, 64, 64), (3, 1, False, 32, 64, 64), (3, 3, False, 32, 64, 64), (3, 3, False, 300, 64, 64),
         (3, 3, False, 1, 256, 256), (3, 3, False, 2, 96, 64), (1, 2, True, 4, 32, 32)]


def _args(a):
    """dummy addresses, every view 160 channels wide, no chunk-major weight copy"""
    def view(v):
        return L.View(DUMMY, 160, v.co) if v is not None else L.View(None, 0, 0)
    return L.conv_args(a, view, lambda field, name: None if field == "wc" else DUMMY)


def _rule(a, roles, cus):
    fused = any(a[k] is not None for k in ("pool", "urot", "unrot", "unrot_smask", "urot_smask", "sign_out", "mask_sign", "upsum_mask_sign", "dst32"))
    return (len(a["taps"]) == 9 and a["H"] == 16 and a["W"] == 16 and a["N"] <= cus and a["Ktot"] in (96, 144) and
            a["c0"] % 48 == 0 and a["c1"] % 48 == 0 and (a["ltw"], a["lth"], a["ltn"], a["kc"]) == (4, 4, 0, 48) and
            ((a["M"], a["Mpad"]) == (96, 96) or ((a["M"], a["Mpad"]) == (144, 160) and a["bf16"] == 1)) and not fused and
            bool(roles & (2 if a["bf16"] else 1)))


@pytest.fixture(autouse=True)
def conv16_reset():
    yield
    L.load().ssdn_conv_set_conv16(-1)


@pytest.mark.parametrize("cin,cout,bs,B,H,W", PLANS)
def test_predicate_claims_only_the_intended_launches(cin, cout, bs, B, H, W):
    lib = L.load()
    cus = 256
    plan = NetPlan("m/", cin, cout, bs, B, H, W, cus=cus, dev_cus=cus)
    convs = [op.a for op in plan.fwd + plan.bwd if op.type == "conv"]
    assert convs
    claimed = {}
    for roles in (3, 1, 2, 0):
        L.check(lib.ssdn_conv_set_conv16(roles))
        for a in convs:
            got = lib.ssdn_conv16_eligible(C.byref(_args(a)))
            assert got == int(_rule(a, roles, cus)), (roles, a["layer"], a["role"], a["N"], a["H"], a["W"])
            if got:
                claimed.setdefault(roles, []).append((a["layer"], a["role"]))
    if (bs, B, H, W) in ((True, 32, 64, 64), (True, 2, 64, 64)):
        both = [("decode_block_3.0", "fwd"), ("decode_block_3.2", "fwd"), ("decode_block_3.2", "dgrad"), ("decode_block_3.0", "dgrad")]
        assert claimed.get(3) == both and claimed.get(1) == both[:2] and claimed.get(2) == both[2:] and 0 not in claimed
    if B > cus:
        assert not claimed
    # the default: the data-gradient role (profiles/conv16_ab.txt)
    L.check(lib.ssdn_conv_set_conv16(-1))
    for a in convs:
        assert lib.ssdn_conv16_eligible(C.byref(_args(a))) == int(_rule(a, 2, cus))
    # mode 0 of ssdn_conv_set_mode is "k_conv always"
    L.check(lib.ssdn_conv_set_mode(0))
    try:
        L.check(lib.ssdn_conv_set_conv16(3))
        assert not any(lib.ssdn_conv16_eligible(C.byref(_args(a))) for a in convs)
    finally:
        L.check(lib.ssdn_conv_set_mode(1))
