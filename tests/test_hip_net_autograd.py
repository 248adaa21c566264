"""GPU: NoiseNetwork under torch autograd -- weight gradients from any upstream gradient and the input gradient
(SSDN_OP_INPUT_GRAD, csrc/input_grad.hip), checked against autograd of the fp32 oracle, teacher-forced against the
restatement of tests/test_net_autograd_cpu.py, through the blind-spot property, and through the semantics torch users rely on."""
import importlib.util
import os

import pytest
import torch
import torch.nn.functional as F

import restate as R
from test_lowering_cpu import _hw_case, flat_params
from test_net_autograd_cpu import restate_input_grad

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-30))


def _cos(a, b):
    a, b = a.reshape(-1).double(), b.reshape(-1).double()
    return float((a * b).sum() / (a.norm() * b.norm() + 1e-30))


def _net(cin, cout, bs, seed=7):
    from ssdn.models.noise_network import NoiseNetwork
    net = NoiseNetwork(cin, cout, blindspot=bs, device="cuda")
    p = R.make_params(cin, cout, bs, seed=seed)
    net.load_state_dict(R.reference_state_dict(p))
    return net, p


def _grads(net):
    return {n: p.grad.detach().cpu().clone() for n, p in net.named_parameters()}


def _oracle(p, x, g, bs):
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    xr = x.clone().requires_grad_(True)
    ref = R.net_forward(leaves, xr, bs)
    (ref * g).sum().backward()
    return ref.detach(), xr.grad, leaves


# x.grad against the fp32 oracle: 1.5 x the worst measured (rel 0.087, cosine 0.99618: the plain 3-channel net at 64x64)
XG_REL, XG_COS = 0.13, 0.994


def _check_against_oracle(net, p, x, g, bs, xgrad, w_cos=0.995):
    ref, rxg, leaves = _oracle(p, x, g, bs)
    bad = []
    for name, prm in net.named_parameters():
        key = name.replace("output_conv", "output_block.4")
        a, rg = prm.grad.detach().cpu(), leaves[key].grad
        # bounds of tests/test_hip_ops.py::test_net_backward_end_to_end (bf16 gradients through 20 layers: LeakyReLU / max-pool branch flips)
        if not (_rel(a, rg) <= 0.13 and _cos(a, rg) >= w_cos):
            bad.append("%s: rel %.3e cos %.5f" % (name, _rel(a, rg), _cos(a, rg)))
    rel, cos = _rel(xgrad, rxg), _cos(xgrad, rxg)
    print("x.grad vs fp32 oracle: rel %.4e cos %.6f" % (rel, cos))
    if not (rel <= XG_REL and cos >= XG_COS):
        bad.append("x.grad: rel %.3e cos %.5f" % (rel, cos))
    assert not bad, "\n".join(bad)
    return ref


def _interpreter_distance(p, x, g, cin, cout):
    """How far fp16 storage alone takes the plain network from the fp32 oracle at this shape: the CPU interpreter (oracle/interp.py) runs the
    planned op list with the device's storage types and fp32 sums, its x.grad is the restatement of SSDN_OP_INPUT_GRAD on its own g_e0 /
    g_d1a.  -> forward rel, worst parameter tensor's rel and cosine, x.grad's rel and cosine, all against autograd of the fp32 oracle."""
    from interp import Interp
    from ssdn.hip import lib as L
    from ssdn.hip.graph import NetPlan, TAPS_PLAIN
    B, _, H, W = x.shape
    plan = NetPlan("m/", cin, cout, False, B, H, W, cus=L.load().ssdn_device_cus())
    it = Interp(plan, flat_params(plan, p), fp16=True)
    it.t["m/in32"] = x
    it.run(plan.pack)
    it.run(plan.fwd)
    it.t["m/g32"] = g
    it.run(plan.bwd)
    ref, rxg, leaves = _oracle(p, x, g, False)
    bf = lambda t: t.to(torch.bfloat16).float()    # noqa: E731
    xg = restate_input_grad(it.t["m/g_e0"], it.t["m/g_d1a"], bf(p["encode_block_1.0.weight"]), bf(p["decode_block_1.0.weight"]), B, 1, TAPS_PLAIN)
    rels, coss = [], []
    for l in plan.layers:
        for sl, rg in ((slice(l.w_off, l.w_off + l.M * l.cin * l.ntaps), leaves[l.name + ".weight"].grad.reshape(-1)),
                       (slice(l.b_off, l.b_off + l.M), leaves[l.name + ".bias"].grad)):
            rels.append(_rel(it.grads[sl], rg))
            coss.append(_cos(it.grads[sl], rg))
    return dict(fwd=_rel(it.t["m/out32"], ref), w_rel=max(rels), w_cos=min(coss), xg_rel=_rel(xg, rxg), xg_cos=_cos(xg, rxg))


# the weight-gradient cosine floor of test_net_backward_end_to_end (0.995) is for its two shapes; the single-channel net, which that test does
# not run, measured 0.99477 on decode_block_5.0 (one output channel: fewer terms to average the bf16 branch flips out): 1.5 x its deficit
# H != W (w_cos None): the bounds above were measured on square input, so these rows are bounded by the reference instead -- 1.5 x the distance
# of the fp16 CPU interpreter from the fp32 oracle at the same shape and input (_interpreter_distance; the worst parameter tensor's for every
# parameter tensor: which activations flip their LeakyReLU branch differs between two fp16 executions, how many does not).
# 32x64: the smallest shape k_conv_thin serves with H != W; 64x96: ragged tiles down to a 2x3 bottom stage.
# measured (device / interpreter, both against the fp32 oracle):
#   32x64: forward rel 6.95e-4 / 6.88e-4; worst parameter tensor rel 0.0797 / 0.0706, cosine 0.99691 / 0.99768; x.grad rel 0.0703 / 0.0703,
#          cosine 0.99753 / 0.99753
#   64x96: forward rel 8.12e-4 / 8.18e-4; worst parameter tensor rel 0.1051 / 0.0982, cosine 0.99447 / 0.99547; x.grad rel 0.0851 / 0.0803,
#          cosine 0.99639 / 0.99677
@pytest.mark.parametrize("cin,cout,bs,B,H,W,w_cos", [_hw_case(*c) for c in [(3, 9, True, 2, 32, 32, 0.995), (3, 3, False, 2, 64, 64, 0.995), (1, 1, True, 2, 32, 32, 0.992),
                                                                            (3, 3, False, 2, 32, 64, None), (3, 3, False, 2, 64, 96, None)]])
def test_end_to_end_against_fp32_autograd(cin, cout, bs, B, H, W, w_cos):
    net, p = _net(cin, cout, bs)
    x = R.hash_tensor((B, cin, H, W), 91, 0, 1)
    g = R.hash_tensor((B, cout, H, W), 92, -1, 1) * 1e-3
    xd = x.cuda().requires_grad_(True)
    out = net(xd)
    assert out.grad_fn is not None
    (out * g.cuda()).sum().backward()
    torch.cuda.synchronize()
    if w_cos is not None:
        ref = _check_against_oracle(net, p, x, g, bs, xd.grad.cpu(), w_cos)
        assert _rel(out.detach().cpu(), ref) <= 5e-3
        return
    d = _interpreter_distance(p, x, g, cin, cout)
    print("fp16 interpreter vs fp32 oracle at %dx%d: %s" % (H, W, d))
    ref, rxg, leaves = _oracle(p, x, g, bs)
    bad, worst = [], [0.0, 1.0]
    for name, prm in net.named_parameters():
        a, rg = prm.grad.detach().cpu(), leaves[name.replace("output_conv", "output_block.4")].grad
        rel, cos = _rel(a, rg), _cos(a, rg)
        worst = [max(worst[0], rel), min(worst[1], cos)]
        if not (rel <= 1.5 * d["w_rel"] and 1 - cos <= 1.5 * (1 - d["w_cos"])):
            bad.append("%s: rel %.3e cos %.5f" % (name, rel, cos))
    rel, cos, fwd = _rel(xd.grad.cpu(), rxg), _cos(xd.grad.cpu(), rxg), _rel(out.detach().cpu(), ref)
    print("device vs fp32 oracle at %dx%d: forward rel %.4e, worst parameter tensor rel %.4e cos %.6f, x.grad rel %.4e cos %.6f" % (
        H, W, fwd, worst[0], worst[1], rel, cos))
    if not (rel <= 1.5 * d["xg_rel"] and 1 - cos <= 1.5 * (1 - d["xg_cos"])):
        bad.append("x.grad: rel %.3e cos %.5f" % (rel, cos))
    if not fwd <= 1.5 * d["fwd"]:
        bad.append("forward: rel %.3e" % fwd)
    assert not bad, "\n".join(bad) + "\ninterpreter: %s" % d


# (plain network at 32x64 / 64x32: the kernel's pixel walk and its halo with H != W; the blind-spot cases stay square: the rotations need it)
@pytest.mark.parametrize("cin,bs,H,W", [pytest.param(3, True, 32, 32, id="3-True"), pytest.param(1, True, 32, 32, id="1-True"), pytest.param(3, False, 32, 32, id="3-False"),
                                        pytest.param(3, False, 32, 64, id="3-False-32x64"), pytest.param(1, False, 64, 32, id="1-False-64x32")])
def test_input_grad_kernel_teacher_forced(cin, bs, H, W):
    """the kernel against the restatement on the device's OWN g_e0 / g_d1a and the bf16-rounded weights it reads: only the fp32 summation
    order differs"""
    B = 2
    net, p = _net(cin, 3, bs, seed=5)
    xd = R.hash_tensor((B, cin, H, W), 31, 0, 1).cuda().requires_grad_(True)
    out = net(xd)
    out.backward(R.hash_tensor((B, 3, H, W), 32, -1, 1).cuda())
    torch.cuda.synchronize()
    eng = net._engines[(B, H, W, True)][0]
    ge, gd = eng.tensor("g_e0").float().cpu(), eng.tensor("g_d1a").float().cpu()
    bf = lambda t: t.to(torch.bfloat16).float()    # noqa: E731
    from ssdn.hip.graph import TAPS_BLIND, TAPS_PLAIN
    want = restate_input_grad(ge, gd, bf(p["encode_block_1.0.weight"]), bf(p["decode_block_1.0.weight"]), B, 4 if bs else 1,
                              TAPS_BLIND if bs else TAPS_PLAIN)
    got = eng.tensor("dx32").cpu()
    assert torch.equal(got, xd.grad.cpu())
    rel = _rel(got, want)
    print("teacher-forced dx32: rel %.3e" % rel)
    assert rel <= 1e-4


def test_blind_spot_property_exact():
    """a one-hot upstream gradient at out[1, :, 13, 17]: the blind-spot net's input gradient is EXACTLY zero at that pixel and in the
    other image; the plain net's is not zero at the centre"""
    B, P, y, x = 2, 32, 13, 17
    g = torch.zeros(B, 3, P, P, device="cuda")
    g[1, :, y, x] = 1.0
    for bs in (True, False):
        net, _ = _net(3, 3, bs, seed=9)
        xd = R.hash_tensor((B, 3, P, P), 41, 0, 1).cuda().requires_grad_(True)
        net(xd).backward(g)
        dx = xd.grad.cpu()
        if bs:
            assert torch.count_nonzero(dx[1, :, y, x]) == 0, dx[1, :, y, x]
            assert torch.count_nonzero(dx[0]) == 0
            nb = torch.stack([dx[1, :, y - 1, x], dx[1, :, y + 1, x], dx[1, :, y, x - 1], dx[1, :, y, x + 1]])
            assert torch.count_nonzero(nb) > 0
        else:
            assert torch.count_nonzero(dx[1, :, y, x]) > 0


def test_autograd_semantics():
    B, P = 2, 32
    net, _ = _net(3, 3, True, seed=13)
    x = R.hash_tensor((B, 3, P, P), 51, 0, 1).cuda()
    g1 = R.hash_tensor((B, 3, P, P), 52, -1, 1).cuda()
    g2 = R.hash_tensor((B, 3, P, P), 53, -1, 1).cuda()

    def pair(g, xg=True):
        xd = x.clone().requires_grad_(xg)
        net(xd).backward(g)
        return xd

    # .grad accumulates over two forward / backward pairs (torch's AccumulateGrad)
    net.zero_grad(set_to_none=True)
    pair(g1)
    G1 = _grads(net)
    net.zero_grad(set_to_none=True)
    pair(g2)
    G2 = _grads(net)
    net.zero_grad(set_to_none=True)
    pair(g1)
    pair(g2)
    G12 = _grads(net)
    for n in G1:
        assert torch.allclose(G12[n], G1[n] + G2[n], rtol=1e-6, atol=0), n

    # frozen parameters: x.grad only
    net.zero_grad(set_to_none=True)
    net.requires_grad_(False)
    xd = pair(g1)
    assert xd.grad is not None and all(p.grad is None for p in net.parameters())
    net.requires_grad_(True)

    # trainable parameters, x without requires_grad: a plan without the input-gradient op
    net._engines.clear()
    net.zero_grad(set_to_none=True)
    pair(g1, xg=False)
    assert (B, P, P, True) not in net._engines
    assert not any(op.type == "input_grad" for op in net._engines[(B, P, P, False)][0].plan.bwd)
    assert torch.equal(_grads(net)["encode_block_1.0.weight"], G1["encode_block_1.0.weight"])

    # a second grad-mode forward of the same shape invalidates the first graph
    xd = x.clone().requires_grad_(True)
    out1 = net(xd)
    out2 = net(xd)
    with pytest.raises(RuntimeError):
        out1.backward(g1)
    out2.backward(g1)

    # an in-place parameter update between forward and backward
    opt = torch.optim.SGD(net.parameters(), lr=1e-3)
    out = net(x.clone().requires_grad_(True))
    opt.step()
    with pytest.raises(RuntimeError):
        out.backward(g1)

    # retain_graph: a second backward of the same graph is bit-identical; double backward raises
    xd = x.clone().requires_grad_(True)
    out = net(xd)
    net.zero_grad(set_to_none=True)
    out.backward(g1, retain_graph=True)
    Ga, xa = _grads(net), xd.grad.clone()
    net.zero_grad(set_to_none=True)
    xd.grad = None
    out.backward(g1)
    Gb = _grads(net)
    assert torch.equal(xd.grad, xa) and all(torch.equal(Ga[n], Gb[n]) for n in Ga)
    xd = x.clone().requires_grad_(True)
    out = net(xd)
    (gx,) = torch.autograd.grad((out * g1).sum(), xd, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()

    # no_grad: the forward-only path, no graph; grad mode computes the same output
    with torch.no_grad():
        o_ng = net(x)
    assert o_ng.grad_fn is None
    o_g = net(x.clone().requires_grad_(True))
    print("grad-mode vs no-grad output: max |diff| %.3e" % float((o_g.detach() - o_ng).abs().max()))
    assert torch.equal(o_g.detach(), o_ng)


def test_full_size_config2():
    """B = 32, 64x64, blind-spot RGB (BASELINE config 2's network): deterministic, exactly linear in the upstream gradient, and x.grad
    within the end-to-end bounds against the fp32 oracle"""
    B, P = 32, 64
    net, p = _net(3, 9, True, seed=11)
    x = R.hash_tensor((B, 3, P, P), 191, 0, 1)
    g = R.hash_tensor((B, 9, P, P), 192, -1, 1) * 1e-3
    xc, gc = x.cuda(), g.cuda()

    def run(scale):
        net.zero_grad(set_to_none=True)
        xd = xc.clone().requires_grad_(True)
        net(xd).backward(gc * scale)
        torch.cuda.synchronize()
        return xd.grad.cpu(), _grads(net)

    dx1, G1 = run(1.0)
    dx1b, G1b = run(1.0)
    assert torch.equal(dx1, dx1b) and all(torch.equal(G1[n], G1b[n]) for n in G1)
    dx2, _ = run(2.0)
    assert torch.equal(dx2, 2 * dx1)
    ref, rxg, _ = _oracle(p, x, g, True)
    rel, cos = _rel(dx1, rxg), _cos(dx1, rxg)
    print("full size x.grad vs fp32 oracle: rel %.4e cos %.6f" % (rel, cos))
    assert rel <= XG_REL and cos >= XG_COS


def test_it_trains():
    """Adam on F.l1_loss(net(noisy), clean) over smooth textures: 30 steps at B = 4, 64x64"""
    spec = importlib.util.spec_from_file_location("convergence_tool", os.path.join(ROOT, "tools", "convergence.py"))
    conv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(conv)
    torch.manual_seed(0)
    from ssdn.models.noise_network import NoiseNetwork
    net = NoiseNetwork(3, 3, blindspot=True, device="cuda")
    clean = conv.textures(4, 64, seed=3).cuda()
    noisy = (clean + 0.1 * R.hash_tensor(tuple(clean.shape), 77, -1.7, 1.7).cuda()).clamp(0, 1)
    opt = torch.optim.Adam(net.parameters(), lr=3e-4)
    losses = []
    for _ in range(30):
        opt.zero_grad(set_to_none=True)
        loss = F.l1_loss(net(noisy), clean)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("l1 losses:", ["%.4f" % v for v in losses])
    first, last = losses[0], sum(losses[-5:]) / 5
    # measured: 0.649 -> 0.051 (mean of the last five steps), 0.079 of the first loss
    assert last < 0.2 * first, (first, last)
