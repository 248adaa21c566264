"""CPU: the planner side of NoiseNetwork's autograd path (NetPlan(input_grad=True)) and a pure-torch restatement of what
SSDN_OP_INPUT_GRAD computes (include/ssdn_hip.h), checked against torch autograd through the oracle's own pieces."""
import pytest
import torch

import restate as R
from ssdn.hip.graph import NetPlan, TAPS_BLIND, TAPS_PLAIN, View


def restate_input_grad(g_e0, g_d1a, w_e, w_d, B, R_, taps):
    """dx[b,c,y,x] = sum_r sum_t [ sum_k g_e0[rB+b, p_r(y,x) - tap_t, k] We[k,c,t] + sum_k g_d1a[rB+b, p_r(y,x) - tap_t, k] Wd[k,96+c,t] ]
    g_e0 [R*B,H,W,48], g_d1a [R*B,H,W,96] (NHWC fp32); w_e [48,C,3,3], w_d [96,96+C,3,3] -> dx [B,C,H,W]."""
    N, H, W, _ = g_e0.shape
    C = w_e.shape[1]
    dx16 = torch.zeros(N, C, H, W, dtype=torch.float64)
    ge, gd = g_e0.double(), g_d1a.double()
    for t, (dy, dx) in enumerate(taps):
        ky, kx = divmod(t, 3)
        # Y[n,c,q] = sum_k g[n,q,k] W[k,c,t];  dx16[n,c,p] += Y[n,c,p - tap]  (zero outside the image)
        y = torch.einsum("nhwk,kc->nchw", ge, w_e[:, :, ky, kx].double()) + torch.einsum("nhwk,kc->nchw", gd, w_d[:, 96:96 + C, ky, kx].double())
        ys, yd = max(0, dy), min(H, H + dy)          # p_y with 0 <= p_y - dy < H
        xs, xd = max(0, dx), min(W, W + dx)
        dx16[:, :, ys:yd, xs:xd] += y[:, :, ys - dy:yd - dy, xs - dx:xd - dx]
    out = torch.zeros(B, C, H, W, dtype=torch.float64)
    for r in range(R_):
        # x16[rB+b] = rotate(x[b], 90 r): the adjoint of a rotation is the opposite rotation
        out += R.rotate(dx16[r * B:(r + 1) * B], (360 - 90 * r) % 360)
    return out.float()


@pytest.mark.parametrize("C,bs", [(1, False), (3, False), (1, True), (3, True)])
def test_restatement_equals_autograd(C, bs):
    """the index algebra of the kernel (rotation map, tap direction, the skip channels 96.. of decode_block_1.0) == autograd of the
    oracle's rotate-stack + conv3x3 of encode_block_1.0 + the skip slice of decode_block_1.0"""
    B, H = 2, 16
    R_ = 4 if bs else 1
    p = R.make_params(C, 3, bs, seed=3)
    w_e, w_d = p["encode_block_1.0.weight"], p["decode_block_1.0.weight"]
    g_e0 = R.hash_tensor((R_ * B, H, H, 48), 11, -1, 1)
    g_d1a = R.hash_tensor((R_ * B, H, H, 96), 12, -1, 1)
    x = R.hash_tensor((B, C, H, H), 13, 0, 1).double().requires_grad_(True)
    xs = torch.cat([R.rotate(x, a) for a in (0, 90, 180, 270)], dim=0) if bs else x
    e = R.conv3x3(xs, w_e.double(), None, bs)
    d = R.conv3x3(xs, w_d[:, 96:].double(), None, bs)
    ((e * g_e0.permute(0, 3, 1, 2).double()).sum() + (d * g_d1a.permute(0, 3, 1, 2).double()).sum()).backward()
    got = restate_input_grad(g_e0, g_d1a, w_e, w_d, B, R_, TAPS_BLIND if bs else TAPS_PLAIN)
    ref = x.grad.float()
    assert float((got - ref).norm() / ref.norm()) <= 1e-5


def _writer(ops, name):
    return [i for i, op in enumerate(ops) if op.type == "conv" and isinstance(op.a.get("dst"), View) and op.a["dst"].t == name]


@pytest.mark.parametrize("C,bs,B,P", [(3, True, 32, 64), (3, True, 2, 32), (1, False, 2, 64), (3, False, 4, 32)])
def test_plan_input_grad_op(C, bs, B, P):
    off = NetPlan("n/", C, C, bs, B, P, P, cus=256)
    on = NetPlan("n/", C, C, bs, B, P, P, cus=256, input_grad=True)
    ig = [i for i, op in enumerate(on.bwd) if op.type == "input_grad"]
    assert len(ig) == 1
    i = ig[0]
    a = on.bwd[i].a
    assert a["g_e0"].t == "n/g_e0" and a["g_d1a"].t == "n/g_d1a" and a["dst"] == "n/dx32"
    assert (a["B"], a["C"], a["H"], a["W"], a["R"]) == (B, C, P, P, 4 if bs else 1)
    assert a["taps"] == (TAPS_BLIND if bs else TAPS_PLAIN)
    assert on.tensors["n/dx32"].kind == "f32" and on.tensors["n/dx32"].shape == (B, C, P, P)
    we, wd = _writer(on.bwd, "n/g_e0"), _writer(on.bwd, "n/g_d1a")
    assert len(we) == 1 and len(wd) == 1 and i == we[0] + 1 and i > wd[0]
    # otherwise the very same plan
    rest = [op for op in on.bwd if op.type != "input_grad"]
    assert [(op.type, op.a) for op in rest] == [(op.type, op.a) for op in off.bwd]
    assert [(op.type, op.a) for op in on.fwd] == [(op.type, op.a) for op in off.fwd]
    assert [(op.type, op.a) for op in on.pack] == [(op.type, op.a) for op in off.pack]
    assert {k: v for k, v in on.tensors.items() if k != "n/dx32"} == off.tensors
    # the scheduled list (chip-wide / per-layer weight-gradient launches) keeps it in place, on the main lane
    out = [(on.bwd[k].type, k, lane) for k, lane in on.bwd_sched]
    pos = [j for j, r in enumerate(out) if r[0] == "input_grad"]
    assert len(pos) == 1 and out[pos[0]][2] == 0              # (the main lane)
    assert [r[1] for r in out].index(we[0]) < pos[0]
    assert len(out) == len(off.bwd_sched) + 1


def test_input_grad_needs_a_training_plan():
    with pytest.raises(ValueError):
        NetPlan("n/", 3, 3, True, 2, 32, 32, cus=256, train=False, input_grad=True)
    # and the default stays the forward-only / training plan of before
    assert not any(op.type == "input_grad" for op in NetPlan("n/", 3, 3, True, 2, 32, 32, cus=256).bwd)


def test_input_grad_rejects_bad_arguments_without_a_gpu():
    """argument errors of SSDN_OP_INPUT_GRAD come back through ssdn_last_error before anything is launched"""
    import ctypes as C
    from ssdn.hip import lib as L
    lib = L.load()
    buf = (C.c_uint16 * 64)()
    w = (C.c_float * 8)()

    def args(**kw):
        a = L.InputGradArgs()
        a.g_e0, a.g_d1a = L.View(C.addressof(buf), 48, 0), L.View(C.addressof(buf), 96, 0)
        a.w_e = a.w_d = a.out = C.addressof(w)
        a.B, a.C, a.H, a.W, a.R, a.ntaps = 1, 3, 32, 32, 4, 9
        for i, (dy, dx) in enumerate(TAPS_BLIND):
            a.dy[i], a.dx[i] = dy, dx
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for kw, msg in ((dict(C=4), b"C = 4"), (dict(C=0), b"C = 0"), (dict(W=64), b"square"), (dict(R=2), b"R = 2"), (dict(H=40, W=40), b"multiples"),
                    (dict(g_e0=L.View(C.addressof(buf), 48, 4)), b"g_e0"), (dict(g_d1a=L.View(C.addressof(buf), 64, 0)), b"g_d1a"),
                    (dict(ntaps=1), b"ntaps")):
        a = args(**kw)
        ops = (L.OpRec * 1)()
        ops[0].type, ops[0].lane, ops[0].args = L.OP["input_grad"], 0, C.cast(C.pointer(a), C.c_void_p)
        assert lib.ssdn_run_ops(ops, 1, None) < 0, kw
        assert msg in lib.ssdn_last_error(), (kw, lib.ssdn_last_error())
