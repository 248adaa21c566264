"""GPU: Denoiser outputs differentiable with respect to the noisy input -- SSDN_OP_HEAD_VJP's g_noisy teacher-forced against float64,
SSDN_OP_INPUT_GRAD's addend, x.grad of the whole route against the model's own NoiseNetwork autograd + a float64 host head, the exact
blind-spot property, bit-identity of everything else, the graph semantics (eval mode included), an Adam run on the image, full size."""
import numpy as np
import pytest
import torch

import restate as R
from test_head_vjp_cpu import VARIANTS, NPAR, head_inputs, upstream
from test_denoiser_input_grad_cpu import head_dy64, oracle_dy
from test_hip_denoiser_autograd import BIT_CASES, DEV, P, batch, run_one, seeded_denoiser, _cos_rel
from head_ops import head_vjp_op

pytestmark = pytest.mark.gpu


# ---- a. teacher-forced head term ------------------------------------------------------------------------------------------------------
# measured on MI355X, max |diff| / max |ref| against float64 autograd (kernel's posterior-mean form): 1 channel <= 1.5e-7; 3 channels
# 1.2e-6 (gauss25 known), 1.9e-6 (const), 1.2e-6 (var), 2.7e-6 (poisson30 known), <= 8.8e-7 (poisson30 const / var).
# Bounds: 1.5x the worst, x max |ref|.
GY_ATOL_C1, GY_ATOL_C3 = 2.3e-7, 4.1e-6


@pytest.mark.parametrize("ch,style,mode", VARIANTS)
def test_head_vjp_g_noisy_vs_float64(ch, style, mode):
    net_out, noisy, npar, raw = head_inputs(ch, style, mode)
    B, H = net_out.shape[0], net_out.shape[2]
    w, gp, gm = upstream(B, ch, H, seed=13 + ch)
    est_raw = raw.mean(dim=(1, 2, 3)) if mode == "var" else raw
    r = head_vjp_op(net_out, noisy, npar, style, mode, est_raw, w, gp, gm)
    want = oracle_dy(net_out, noisy, npar, style, mode, raw, w, gp, gm, kernel_pme=True)
    got = r["g_noisy"].cpu().double()
    err = float((got - want).abs().max() / want.abs().max())
    print("g_noisy vs fp64 autograd %d/%s/%s: max |diff| / max |ref| = %.3e" % (ch, style, mode, err))
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=2e-4, atol=(GY_ATOL_C1 if ch == 1 else GY_ATOL_C3) * float(want.abs().max()))
    g64 = head_dy64(net_out, noisy, npar, style, mode, est_raw.double() if est_raw is not None else None, w, gp, gm)
    np.testing.assert_allclose(got.numpy(), g64.numpy(), rtol=2e-4, atol=(GY_ATOL_C1 if ch == 1 else GY_ATOL_C3) * float(g64.abs().max()))
    # the other outputs are those of the launch without g_noisy, bit for bit
    r0 = head_vjp_op(net_out, noisy, npar, style, mode, est_raw, w, gp, gm, g_noisy=False)
    for k in ("g_net_out", "partial", "g_est", "g_sig", "gmax"):
        if r0[k] is not None:
            assert torch.equal(r[k], r0[k]) or (k == "g_net_out" and torch.equal(r[k].nan_to_num(7.0), r0[k].nan_to_num(7.0))), k


@pytest.mark.parametrize("ch,style,mode", [(3, "gauss25", "known"), (1, "poisson30", "const"), (3, "gauss25", "var")])
def test_head_vjp_keep_path_writes_g_noisy_only(ch, style, mode):
    net_out, noisy, npar, raw = head_inputs(ch, style, mode, B=3)
    B, H = net_out.shape[0], net_out.shape[2]
    est_raw = raw.mean(dim=(1, 2, 3)) if mode == "var" else raw
    w = torch.full((B,), 1.0 / B)
    w[1] = 0.5                                              # sample 1 is not the forward's d mean(LOSS): it is recomputed
    g_init = torch.full((B, net_out.shape[1], H, H), 7.0)
    p_init = torch.full((B, 2, 2), 3.0)
    r = head_vjp_op(net_out, noisy, npar, style, mode, est_raw, w, None, None, keep=1, g_init=g_init, partial_init=p_init)
    full = head_vjp_op(net_out, noisy, npar, style, mode, est_raw, w, None, None, keep=0)
    for b in (0, 2):                                        # kept samples: gradient and partials untouched, g_noisy written
        assert torch.equal(r["g_net_out"][b].cpu(), g_init[b]) and torch.equal(r["partial"][b].cpu(), p_init[b])
    assert torch.equal(r["g_net_out"][1], full["g_net_out"][1])
    assert torch.equal(r["g_noisy"], full["g_noisy"]) and torch.isfinite(r["g_noisy"]).all()
    assert float(r["g_noisy"].abs().max()) > 0


# ---- b. SSDN_OP_INPUT_GRAD's addend ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,bs", [(3, True), (1, False)])
def test_input_grad_addend(cin, bs):
    from ssdn.hip import lib as L
    from ssdn.models.noise_network import NoiseNetwork
    B, Psz = 2, 32
    net = NoiseNetwork(cin, 3, blindspot=bs, device="cuda")
    net.load_state_dict(R.reference_state_dict(R.make_params(cin, 3, bs, seed=5)))
    xd = R.hash_tensor((B, cin, Psz, Psz), 31, 0, 1).cuda().requires_grad_(True)
    net(xd).backward(R.hash_tensor((B, 3, Psz, Psz), 32, -1, 1).cuda())
    torch.cuda.synchronize()
    eng = net._engines[(B, Psz, Psz, True)][0]
    a = L.InputGradArgs.from_buffer_copy(eng.input_grad_args)
    assert a.add is None
    out0 = torch.full((B, cin, Psz, Psz), float("nan"), device=DEV)
    a.out = P(out0)
    run_one("input_grad", a)
    add = R.hash_tensor((B, cin, Psz, Psz), 33, -1, 1).cuda()
    out1 = torch.full_like(out0, float("nan"))
    a.out, a.add = P(out1), P(add)
    run_one("input_grad", a)
    assert torch.equal(out1, out0 + add)
    alias = add.clone()                                     # add aliasing out
    a.out = a.add = P(alias)
    run_one("input_grad", a)
    assert torch.equal(alias, out0 + add)


# ---- c. end to end against the model's own NoiseNetwork autograd + the float64 host head ------------------------------------------
# measured on MI355X, 1 - cosine / relative L2 error of x.grad, B 4, 32x32: 6.6e-6 / 3.6e-3 (gauss25 known), 6.1e-6 / 3.5e-3 (poisson30
# const), 9.2e-6 / 4.3e-3 (gauss25 var), 1 channel 1e-16 / 3.6e-8; n2c and n2v exact (no head term: the same kernels on both routes).
# Full size (B 32, 64x64, test h): 1.6e-5 / 5.7e-3 (known), 1.8e-5 / 6.0e-3 (var).  The 3-channel differences are the fp32 head (kernel's
# posterior-mean form) against the float64 reference head, carried through the bf16 data gradients.  Bounds: 1.5x the worst of both.
XG_1MCOS, XG_REL = 2.7e-5, 9e-3

E2E_CASES = [("ssdn", "gauss25", "known", 3), ("ssdn", "poisson30", "const", 3), ("ssdn", "gauss25", "var", 3), ("ssdn", "gauss25", "known", 1),
             ("n2c", "gauss25", "known", 3), ("n2v", "gauss25", "known", 3)]


def _upstream_dev(alg, B, ch, Psz, seed):
    w, gp, gm = upstream(B, ch, Psz, seed=seed)
    return w.to(DEV), gp.to(DEV) * 1e-2, (gm.to(DEV) * 1e-2 if alg == "ssdn" else None)


def _route_loss(alg, res, w, gp, gm):
    from ssdn.params import PipelineOutput as PO
    B = w.shape[0]
    L = (res[PO.LOSS].view(B) * w).sum() + (res[PO.IMG_DENOISED] * gp).sum()
    if alg == "ssdn":
        L = L + (res[PO.IMG_MU] * gm).sum()
    return L


def reference_x_grad(d, alg, style, mode, data, w, gp, gm):
    """x.grad through the model's NoiseNetwork autograd (and the sigma network's, var) plus a float64 host head whose noisy image is a
    leaf of its own: the sum of both leaves' gradients"""
    from ssdn.denoiser import Denoiser
    from ssdn.datasets import NoisyDataset
    noisy, ref = data[0], data[1]
    B, ch = noisy.shape[:2]
    xr = noisy.detach().clone().requires_grad_(True)
    out = d.get_model(Denoiser.MODEL, False)(xr)
    y64 = noisy.detach().cpu().double().requires_grad_(True)
    if alg == "ssdn":
        est = None
        if mode == "var":
            est = d.get_model(Denoiser.SIGMA_ESTIMATOR, False)(xr).mean(dim=(2, 3), keepdim=True).cpu().double()
        elif mode == "const":
            est = d.l_params[Denoiser.ESTIMATED_SIGMA].detach().cpu().double()
        npar = torch.full((B, 1, 1, 1), NPAR[style], dtype=torch.float64)
        o = R.ssdn_head(out.cpu().double(), y64, npar, style, mode, est)
        L = (o["loss"].view(B) * w.cpu().double()).sum() + (o["out"] * gp.cpu().double()).sum() + (o["out_mu"] * gm.cpu().double()).sum()
    else:
        o64 = out.cpu().double()
        if alg == "n2v":
            loss = R.mask_mse_loss(data[2][NoisyDataset.Metadata.MASK_COORDS], o64, ref.cpu().double())
        else:
            loss = R.mse_loss(o64, ref.cpu().double())
        L = (loss.view(B) * w.cpu().double()).sum() + (o64 * gp.cpu().double()).sum()
    L.backward()
    torch.cuda.synchronize()
    return xr.grad.cpu().double() + (y64.grad if y64.grad is not None else 0)


def _x_grad_route(d, alg, data, w, gp, gm):
    x = data[0].detach().clone().requires_grad_(True)
    res = d.run_pipeline([x] + list(data[1:]))
    _route_loss(alg, res, w, gp, gm).backward()
    torch.cuda.synchronize()
    return x, res


@pytest.mark.parametrize("alg,style,mode,ch", E2E_CASES)
def test_end_to_end_x_grad_vs_network_autograd(alg, style, mode, ch):
    B, Psz = 4, 32
    d = seeded_denoiser(alg, style, mode, ch)
    data = batch(alg, style, ch, B, Psz)
    w, gp, gm = _upstream_dev(alg, B, ch, Psz, seed=23)
    want = reference_x_grad(d, alg, style, mode, data, w, gp, gm)
    x, _ = _x_grad_route(d, alg, data, w, gp, gm)
    assert x.grad is not None and x.grad.shape == x.shape and x.grad.dtype == x.dtype
    got = x.grad.cpu().double()
    cos, rel = _cos_rel(got.reshape(-1), want.reshape(-1))
    print("x.grad end to end %s/%s/%s/C%d: 1 - cosine %.3e, rel err %.3e" % (alg, style, mode, ch, 1 - cos, rel))
    assert torch.isfinite(got).all()
    assert 1 - cos <= XG_1MCOS and rel <= XG_REL, (cos, rel)


# ---- d. blind-spot exactness ----------------------------------------------------------------------------------------------------------
def test_blind_spot_x_grad_exact():
    from ssdn.hip import lib as L
    from ssdn.hip.engine import STYLE, MODE
    from ssdn.params import PipelineOutput as PO
    B, Psz, ch, yy, xx = 2, 32, 3, 13, 17
    d = seeded_denoiser("ssdn", "gauss25", "known", ch)
    data = batch("ssdn", "gauss25", ch, B, Psz)
    x = data[0].detach().clone().requires_grad_(True)
    res = d.run_pipeline([x] + data[1:])
    g = torch.zeros(B, ch, Psz, Psz, device=DEV)
    g[1, :, yy, xx] = torch.tensor([0.7, -1.3, 0.4], device=DEV)
    res[PO.IMG_DENOISED].backward(g)
    torch.cuda.synchronize()
    assert torch.count_nonzero(x.grad[0]) == 0
    # the network's share at the pixel is exactly 0: x.grad there is the head term of a teacher-forced launch on the engine's own data
    eng = d._last_train_engine
    gy = torch.full((B, ch, Psz, Psz), float("nan"), device=DEV)
    gno = torch.zeros(B, ch + ch * (ch + 1) // 2, Psz, Psz, device=DEV)
    partial = torch.zeros(B, eng.nchunks, 2, device=DEV)
    gmax = torch.zeros(4, dtype=torch.int32, device=DEV)
    a = L.HeadVjpArgs(P(eng.main.tensor("out32")), P(eng.inp), P(eng.noise_param), None, B, ch, Psz, Psz, STYLE["gauss"], MODE["known"],
                      None, P(g), None, 0, eng.nchunks, P(gno), P(partial), P(gmax), None, None, None)
    a.g_noisy = P(gy)
    run_one("head_vjp", a)
    assert torch.equal(x.grad[1, :, yy, xx], gy[1, :, yy, xx])
    assert torch.count_nonzero(gy[1, :, yy, xx]) > 0


# ---- e. bit-identity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [41, 4])
@pytest.mark.parametrize("alg,style,mode,ch", BIT_CASES)
def test_parameter_grads_and_outputs_bit_identical_with_x_grad(alg, style, mode, ch, B):
    from ssdn.params import PipelineOutput as PO
    d = seeded_denoiser(alg, style, mode, ch)
    data = batch(alg, style, ch, B, 32)
    w, gp, gm = _upstream_dev(alg, B, ch, 32, seed=29)
    keys = [PO.LOSS, PO.IMG_DENOISED] + ([PO.IMG_MU] if alg == "ssdn" else [])
    res = d.run_pipeline(data)
    _route_loss(alg, res, w, gp, gm).backward()
    torch.cuda.synchronize()
    g_ref = d.flat_grad.clone()
    x, res2 = _x_grad_route(d, alg, data, w, gp, gm)
    assert torch.equal(d.flat_grad, g_ref), "%d of %d gradient elements differ" % (int((d.flat_grad != g_ref).sum()), g_ref.numel())
    for k in keys:
        assert torch.equal(res2[k].detach(), res[k].detach()), k
    assert torch.isfinite(x.grad).all()
    # two backward passes of one graph
    x = data[0].detach().clone().requires_grad_(True)
    res3 = d.run_pipeline([x] + data[1:])
    L3 = _route_loss(alg, res3, w, gp, gm)
    L3.backward(retain_graph=True)
    torch.cuda.synchronize()
    g1 = x.grad.clone()
    x.grad = None
    L3.backward()
    torch.cuda.synchronize()
    assert torch.equal(x.grad, g1)
    assert torch.equal(d.flat_grad, g_ref)


# ---- f. semantics ---------------------------------------------------------------------------------------------------------------------
def test_input_grad_semantics():
    from ssdn.params import PipelineOutput as PO
    B, Psz = 2, 32
    d = seeded_denoiser("ssdn", "gauss25", "known", 3)
    data = batch("ssdn", "gauss25", 3, B, Psz)
    d.train_step(data, lr=0.0)                              # creates the training engine of this shape (input_buffer())
    w, gp, gm = _upstream_dev("ssdn", B, 3, Psz, seed=37)
    # the engines' input buffers never join the caller's graph
    x = data[0].detach().clone().requires_grad_(True)
    res = d.run_pipeline([x] + data[1:])
    for slot in d._engines.values():
        assert not slot[0].inp.requires_grad and slot[0].inp.grad_fn is None
    assert not d.input_buffer(B, Psz, Psz).requires_grad
    _route_loss("ssdn", res, w, gp, gm).backward()
    torch.cuda.synchronize()
    g_dev = x.grad.clone()
    # a CPU input gets a CPU .grad (same values)
    xc = data[0].detach().cpu().clone().requires_grad_(True)
    _route_loss("ssdn", d.run_pipeline([xc] + data[1:]), w, gp, gm).backward()
    assert xc.grad.device.type == "cpu" and torch.equal(xc.grad, g_dev.cpu())
    # .grad accumulates across two forward / backward pairs
    _route_loss("ssdn", d.run_pipeline([xc] + data[1:]), w, gp, gm).backward()
    assert torch.equal(xc.grad, g_dev.cpu() + g_dev.cpu())
    # eval(): a graph with x.requires_grad, outputs equal to the no_grad eval outputs; none without it
    train_out = d.run_pipeline(data)                        # the training forward the planned route acts on
    d.backward()
    torch.cuda.synchronize()
    g_train = d.flat_grad.clone()
    d.eval()
    with torch.no_grad():
        ev = d.run_pipeline(data)
    xe = data[0].detach().clone().requires_grad_(True)
    ev2 = d.run_pipeline([xe] + data[1:])
    for k in (PO.LOSS, PO.IMG_DENOISED, PO.IMG_MU):
        assert ev2[k].requires_grad, k
        assert torch.equal(ev2[k].detach(), ev[k]), k
    for k in (PO.NOISE_STD_DEV, PO.MODEL_STD_DEV):
        assert not ev2[k].requires_grad and torch.equal(ev2[k], ev[k]), k
    ev3 = d.run_pipeline(data)
    assert not any(ev3[k].requires_grad for k in (PO.LOSS, PO.IMG_DENOISED, PO.IMG_MU))
    assert not d._last_train_engine.input_grad
    ev2[PO.IMG_DENOISED].sum().backward()
    torch.cuda.synchronize()
    assert xe.grad is not None and float(xe.grad.abs().max()) > 0
    # Denoiser.backward() and optimizer_step() still act on the training forward
    d.backward()
    torch.cuda.synchronize()
    assert torch.equal(d.flat_grad, g_train)
    p0 = d.flat.clone()
    d.optimizer_step(1e-3)
    torch.cuda.synchronize()
    assert not torch.equal(d.flat, p0)
    # a stale graph still raises: another input-gradient run of the same shape since
    a = d.run_pipeline([xe] + data[1:])
    d.run_pipeline([xe] + data[1:])
    with pytest.raises(RuntimeError, match="later training forward"):
        a[PO.IMG_DENOISED].sum().backward()
    # train_step: no graph, x.grad untouched
    d.train()
    xt = data[0].detach().clone().requires_grad_(True)
    o = d.train_step([xt] + data[1:], lr=0.0)
    assert not any(o[k].requires_grad for k in (PO.LOSS, PO.IMG_DENOISED, PO.IMG_MU))
    assert xt.grad is None


# ---- g. capability: optimising the image through a frozen denoiser in eval() ----------------------------------------------------------
def test_adam_on_the_input_in_eval_descends():
    from ssdn.params import PipelineOutput as PO
    from ssdn.datasets import NoisyDataset
    B, Psz = 2, 32
    d = seeded_denoiser("ssdn", "gauss25", "known", 3)
    d.eval()
    for p in d.parameters():
        p.requires_grad_(False)
    data = batch("ssdn", "gauss25", 3, B, Psz, seed=4)
    target = data[2][NoisyDataset.Metadata.CLEAN].to(DEV)
    flat0 = d.flat.clone()
    x = data[0].detach().clone().requires_grad_(True)
    opt = torch.optim.Adam([x], lr=1e-2)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss = ((d.run_pipeline([x] + data[1:])[PO.IMG_DENOISED] - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("image-space MSE over 30 Adam steps: %.5f -> %.5f" % (losses[0], losses[-1]))
    assert all(np.isfinite(losses)) and losses[-1] < 0.5 * losses[0], losses
    assert torch.equal(d.flat, flat0)


# ---- h. full size ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["known", "var"])
def test_full_size_x_grad(mode):
    B, Psz, ch = 32, 64, 3
    d = seeded_denoiser("ssdn", "gauss25", mode, ch)
    data = batch("ssdn", "gauss25", ch, B, Psz, seed=7)
    w, gp, gm = _upstream_dev("ssdn", B, ch, Psz, seed=31)
    want = reference_x_grad(d, "ssdn", "gauss25", mode, data, w, gp, gm)
    x, _ = _x_grad_route(d, "ssdn", data, w, gp, gm)
    got = x.grad.cpu().double()
    assert torch.isfinite(got).all()
    cos, rel = _cos_rel(got.reshape(-1), want.reshape(-1))
    print("x.grad full size gauss25/%s: 1 - cosine %.3e, rel err %.3e" % (mode, 1 - cos, rel))
    assert 1 - cos <= XG_1MCOS and rel <= XG_REL, (cos, rel)
