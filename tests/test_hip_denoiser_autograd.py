"""GPU: Denoiser outputs under autograd for any upstream gradient -- SSDN_OP_HEAD_VJP / SSDN_OP_MSE_VJP teacher-forced against float64
autograd of the oracle head, the whole route against the model's own NoiseNetwork autograd + a float64 torch head, the bit-identity of
torch.mean(LOSS).backward() with Denoiser.backward(), linearity, the graph semantics, an Adam run on a posterior-mean loss, full size."""
import numpy as np
import pytest
import torch

import restate as R
from test_head_vjp_cpu import VARIANTS, NPAR, head_inputs, upstream, head_vjp64, oracle_vjp, mse_vjp64
from test_hip_denoiser import make_denoiser
from head_ops import DEV, P, head_vjp_op, run_one          # (DEV, P and run_one: the other GPU test modules import them from here)

pytestmark = pytest.mark.gpu


def _cmp(a, b, rtol, atol_rel, what=""):
    b = b.detach().cpu().double()
    a = a.detach().cpu().double().reshape(b.shape)
    print("%s max |diff| / max |ref| = %.3e" % (what, float((a - b).abs().max() / b.abs().max())))
    np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=rtol, atol=atol_rel * float(b.abs().max()))


# The 3-channel posterior-mean term solves with T = Sx + Sn + 2 eps I in fp32, as the forward does; where Sx is near singular a few
# elements of dL/dnet_out are off by more than rel 2e-4.  Measured on MI355X, max |diff| / max |ref|: 1 channel <= 1.9e-7; 3 channels
# 2.8e-5 (gauss25 known), 2.4e-5 (const), 5.8e-6 (var), <= 4.3e-6 (poisson30).  atol: 1.5x the worst, x max |ref|.
ATOL_C3 = 4.5e-5


# ---- 1. teacher-forced ops ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ch,style,mode", VARIANTS)
def test_head_vjp_op_vs_float64_autograd(ch, style, mode):
    net_out, noisy, npar, raw = head_inputs(ch, style, mode)
    B, H = net_out.shape[0], net_out.shape[2]
    w, gp, gm = upstream(B, ch, H, seed=11 + ch)
    est_raw = raw.mean(dim=(1, 2, 3)) if mode == "var" else raw
    r = head_vjp_op(net_out, noisy, npar, style, mode, est_raw, w, gp, gm, g_noisy=False)
    gno, g_est, g_sig, gmax = r["g_net_out"], r["g_est"], r["g_sig"], r["gmax"]
    og, oraw = oracle_vjp(net_out, noisy, npar, style, mode, raw, w, gp, gm)
    _cmp(gno, og, 2e-4, 1e-6 if ch == 1 else ATOL_C3, "op vs fp64 autograd %d/%s/%s:" % (ch, style, mode))
    assert float(np.int32(gmax[0].item()).view(np.float32)) == pytest.approx(float(gno.abs().max()), rel=1e-6)
    if mode == "const":
        _cmp(g_est[:1], oraw.reshape(1), 2e-4, 1e-9)
    if mode == "var":
        _cmp(g_sig, oraw, 2e-4, 1e-10)
    # and the CPU restatement (tests/test_head_vjp_cpu.py) of the very closed forms the kernel evaluates
    g64, _ = head_vjp64(net_out, noisy, npar, style, mode, est_raw.double() if est_raw is not None else None, w, gp, gm)
    _cmp(gno, g64, 2e-4, 1e-6 if ch == 1 else ATOL_C3)


@pytest.mark.parametrize("masked", [False, True])
def test_mse_vjp_op_vs_float64(masked):
    from ssdn.hip import lib as L
    B, C, H = 3, 3, 16
    out = R.hash_tensor((B, C, H, H), 51, 0, 1)
    ref = R.hash_tensor((B, C, H, H), 52, 0, 1)
    w, gp, _ = upstream(B, C, H, seed=3, g_mu=False)
    c0 = torch.randint(0, H, (12, 2), generator=torch.Generator().manual_seed(5))
    c0[5] = c0[2]
    c0[9] = c0[2]                                          # duplicates count three times
    for ww, gg in ((w, gp), (w, None), (None, gp)):
        g = torch.full((B, C, H, H), float("nan"), device=DEV)
        gmax = torch.zeros(4, dtype=torch.int32, device=DEV)
        dd = [t.to(DEV).contiguous() if t is not None else None for t in (out, ref, c0, ww, gg)]
        run_one("mse_vjp", L.MseVjpArgs(P(dd[0]), P(dd[1]), P(dd[2]), 12, int(masked), B, C, H, H, 0, P(dd[3]), P(dd[4]), P(g), P(gmax)))
        _cmp(g, mse_vjp64(out, ref, ww, gg, c0[None] if masked else None), 1e-5, 1e-7)


# ---- helpers for the Denoiser-level tests ----------------------------------------------------------------------------------------------
def batch(alg, style, ch, B, Psz, seed=0):
    from ssdn.datasets import NoisyDataset
    MD = NoisyDataset.Metadata
    clean = R.hash_tensor((B, ch, Psz, Psz), 161 + seed, 0, 1)
    noisy = torch.clamp(clean + R.hash_tensor((B, ch, Psz, Psz), 162 + seed, -1, 1) * 0.17, 0, 1)
    ref = clean if alg != "n2v" else torch.clamp(clean + R.hash_tensor((B, ch, Psz, Psz), 163 + seed, -1, 1) * 0.17, 0, 1)
    meta = {MD.CLEAN: clean, MD.INPUT_NOISE_VALUES: torch.full((B, 1, 1, 1), NPAR[style])}
    if alg == "n2v":
        meta[MD.MASK_COORDS] = R.hash_tensor((B, 64, 2), 164 + seed, 0, Psz).long()
    return [noisy.to(DEV), ref.to(DEV), meta]


def seeded_denoiser(alg, style, mode, ch):
    from ssdn.denoiser import Denoiser
    d = make_denoiser(alg, style, mode, ch)
    cout = ch + ch * (ch + 1) // 2 if alg == "ssdn" else ch
    d.get_model(Denoiser.MODEL, False).load_state_dict(R.reference_state_dict(R.make_params(ch, cout, alg == "ssdn", seed=5)))
    if mode == "var":
        d.get_model(Denoiser.SIGMA_ESTIMATOR, False).load_state_dict(R.reference_state_dict(R.make_params(ch, 1, False, seed=6)))
    if mode == "const":
        with torch.no_grad():
            d.l_params[Denoiser.ESTIMATED_SIGMA].fill_(1.7)
    d.mark_dirty()
    d.train()
    return d


def _cos_rel(a, b):
    a, b = a.double(), b.double()
    return float((a @ b) / (a.norm() * b.norm())), float((a - b).norm() / b.norm())


def _flat_param_grads(d):
    """the parameters' .grad (as torch's AccumulateGrad left them) in the flat buffer's layout"""
    f = torch.zeros_like(d.flat)
    for p, (off, n, _) in zip(d.parameters(), d._param_slices()):
        if p.grad is not None:
            f[off:off + n] = p.grad.reshape(-1)
    return f


# ---- 2. end to end vs the NoiseNetwork autograd route ------------------------------------------------------------------------------------
# measured on MI355X (B 4, 32x32, 3 channels): relative L2 error 4.3e-4 (gauss25 known), 1.49e-3 (poisson30 const), 9.0e-4 (gauss25 var);
# 1 - cosine 9.3e-8, 1.11e-6, 4.1e-7.  Bounds: 1.5x the worst.
E2E_1MCOS, E2E_REL = 1.7e-6, 2.3e-3


@pytest.mark.parametrize("style,mode", [("gauss25", "known"), ("poisson30", "const"), ("gauss25", "var")])
def test_end_to_end_any_upstream_vs_network_autograd(style, mode):
    from ssdn.denoiser import Denoiser
    from ssdn.params import PipelineOutput as PO
    ch, B, Psz = 3, 4, 32
    d = seeded_denoiser("ssdn", style, mode, ch)
    data = batch("ssdn", style, ch, B, Psz)
    w, gp, gm = upstream(B, ch, Psz, seed=21)
    w, gp, gm = w.to(DEV), gp.to(DEV) * 1e-2, gm.to(DEV) * 1e-2
    # reference: the model's own NoiseNetwork autograd (HIP backward lists) + the float64 torch head on the host
    for p in d.parameters():
        p.grad = None
    noisy = data[0]
    out = d.get_model(Denoiser.MODEL, False)(noisy)
    est = None
    if mode == "var":
        est = d.get_model(Denoiser.SIGMA_ESTIMATOR, False)(noisy).mean(dim=(2, 3), keepdim=True).cpu().double()
    elif mode == "const":
        est = d.l_params[Denoiser.ESTIMATED_SIGMA].cpu().double()
    npar = torch.full((B, 1, 1, 1), NPAR[style], dtype=torch.float64)
    o = R.ssdn_head(out.cpu().double(), noisy.cpu().double(), npar, style, mode, est)
    L = (o["loss"].view(B) * w.cpu().double()).sum() + (o["out"] * gp.cpu().double()).sum() + (o["out_mu"] * gm.cpu().double()).sum()
    L.backward()
    torch.cuda.synchronize()
    want = _flat_param_grads(d)
    for p in d.parameters():
        p.grad = None
    # the Denoiser route
    res = d.run_pipeline(data)
    L2 = (res[PO.LOSS].view(B) * w).sum() + (res[PO.IMG_DENOISED] * gp).sum() + (res[PO.IMG_MU] * gm).sum()
    L2.backward()
    torch.cuda.synchronize()
    got = d.flat_grad.clone()
    cos, rel = _cos_rel(got, want)
    print("end-to-end %s/%s: 1 - cosine %.3e, rel err %.3e" % (style, mode, 1 - cos, rel))
    assert torch.isfinite(got).all()
    assert 1 - cos <= E2E_1MCOS and rel <= E2E_REL, (cos, rel)
    if mode == "const":                     # the learnable sigma's gradient on its own
        o_ = d._n_main + d._n_sig
        assert float(got[o_]) == pytest.approx(float(want[o_]), rel=2e-2, abs=1e-6)


# ---- 3. bit-identity of torch.mean(LOSS).backward() with Denoiser.backward() ------------------------------------------------------------
BIT_CASES = [("ssdn", "gauss25", "known", 3), ("ssdn", "poisson30", "const", 3), ("ssdn", "gauss25", "var", 3),
             ("n2c", "gauss25", "known", 1), ("n2v", "gauss25", "known", 3)]


@pytest.mark.parametrize("B", [41, 4])
@pytest.mark.parametrize("alg,style,mode,ch", BIT_CASES)
def test_mean_loss_backward_is_bit_identical_to_planned_backward(alg, style, mode, ch, B):
    from ssdn.params import PipelineOutput as PO
    d = seeded_denoiser(alg, style, mode, ch)
    data = batch(alg, style, ch, B, 32)
    out = d.run_pipeline(data)
    d.backward()
    torch.cuda.synchronize()
    g_ref = d.flat_grad.clone()
    loss_ref = out[PO.LOSS].detach().clone()
    d.flat_grad.zero_()
    out = d.run_pipeline(data)
    torch.mean(out[PO.LOSS]).backward()
    torch.cuda.synchronize()
    assert torch.equal(out[PO.LOSS].detach(), loss_ref)
    assert torch.equal(d.flat_grad, g_ref), "%d of %d gradient elements differ" % (int((d.flat_grad != g_ref).sum()), g_ref.numel())
    # the forward's LOSS values in the engine (what accumulate_metrics reads) are the same after the VJP
    assert torch.equal(d._last_train_engine.loss, loss_ref)


# ---- 4. linearity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg,style,mode,ch", [("ssdn", "poisson30", "const", 3), ("ssdn", "gauss25", "var", 3), ("n2v", "gauss25", "known", 3)])
def test_vjp_is_linear_in_the_upstream_gradient(alg, style, mode, ch):
    from ssdn.params import PipelineOutput as PO
    B = 4
    d = seeded_denoiser(alg, style, mode, ch)
    data = batch(alg, style, ch, B, 32)
    w = torch.tensor([0.7, -0.3, 1.9, 0.45], device=DEV)

    def grad_for(wv):
        out = d.run_pipeline(data)
        (out[PO.LOSS].view(B) * wv).sum().backward()
        torch.cuda.synchronize()
        return d.flat_grad.clone()
    full = grad_for(w)
    parts = sum(grad_for(w * torch.nn.functional.one_hot(torch.tensor(b), B).to(DEV, torch.float32)) for b in range(B))
    cos, rel = _cos_rel(parts, full)
    assert cos >= 0.9999 and rel <= 1e-2, (cos, rel)      # (the backward pass rounds data gradients to bf16: not exactly linear)
    scaled = grad_for(w * 4.0)                           # a power of two scales every intermediate exactly
    np.testing.assert_allclose(scaled.cpu().numpy(), (4.0 * full).cpu().numpy(), rtol=1e-6, atol=1e-6 * float(full.abs().max()) * 4)


# ---- 5. semantics ---------------------------------------------------------------------------------------------------------------------
def test_which_outputs_carry_a_graph_and_stale_graphs_raise():
    from ssdn.params import PipelineOutput as PO
    d = seeded_denoiser("ssdn", "gauss25", "known", 3)
    data = batch("ssdn", "gauss25", 3, 2, 32)
    out = d.run_pipeline(data)
    for k in (PO.LOSS, PO.IMG_DENOISED, PO.IMG_MU):
        assert out[k].requires_grad and out[k].grad_fn is not None, k
    for k in (PO.NOISE_STD_DEV, PO.MODEL_STD_DEV):
        assert not out[k].requires_grad, k
    with torch.no_grad():
        o2 = d.run_pipeline(data)
    assert not any(o2[k].requires_grad for k in (PO.LOSS, PO.IMG_DENOISED, PO.IMG_MU))
    d.eval()
    o3 = d.run_pipeline(data)
    assert not any(o3[k].requires_grad for k in (PO.LOSS, PO.IMG_DENOISED, PO.IMG_MU))
    d.train()
    o4 = d.train_step(data, lr=0.0)
    assert not any(o4[k].requires_grad for k in (PO.LOSS, PO.IMG_DENOISED, PO.IMG_MU))
    # stale: another training forward of the same shape (run_pipeline, then train_step) since the graph was made
    a = d.run_pipeline(data)
    d.run_pipeline(data)
    with pytest.raises(RuntimeError, match="later training forward"):
        a[PO.IMG_DENOISED].sum().backward()
    b = d.run_pipeline(data)
    d.train_step(data, lr=0.0)
    with pytest.raises(RuntimeError, match="later training forward"):
        torch.mean(b[PO.LOSS]).backward()
    # an eval run in between does not make it stale
    c = d.run_pipeline(data)
    with torch.no_grad():
        d.eval()
        d.run_pipeline(data)
        d.train()
    c[PO.IMG_MU].sum().backward()
    torch.cuda.synchronize()
    assert float(d.flat_grad.abs().max()) > 0
    # the planned route (Denoiser.backward) consumes its forward: the images are plain tensors again, LOSS keeps its graph
    e = d.run_pipeline(data)
    d.backward()
    assert not e[PO.IMG_DENOISED].requires_grad and not e[PO.IMG_MU].requires_grad
    assert e[PO.IMG_DENOISED].cpu().numpy().shape == (2, 3, 32, 32)
    torch.mean(e[PO.LOSS]).backward()


def test_forward_sum_backward_const_mode():
    from ssdn.denoiser import Denoiser
    d = seeded_denoiser("ssdn", "gauss25", "const", 3)
    x = batch("ssdn", "gauss25", 3, 2, 32)[0]
    y = d(x)
    assert y.requires_grad
    n = d._n_main + d._n_sig + 1                        # (the flat buffer's padding is nobody's gradient)
    d.flat_grad.fill_(float("nan"))
    y.sum().backward()
    torch.cuda.synchronize()
    assert torch.isfinite(d.flat_grad[:n]).all() and float(d.flat_grad[:n].abs().max()) > 0
    s = d.l_params[Denoiser.ESTIMATED_SIGMA]
    assert s.grad is not None and float(s.grad.abs()) > 0        # the posterior mean depends on the learnt sigma


# ---- 6. capability: a supervised fine-tune on the posterior mean ------------------------------------------------------------------------
def test_adam_on_posterior_mean_loss_descends():
    from ssdn.params import PipelineOutput as PO
    from ssdn.datasets import NoisyDataset
    d = seeded_denoiser("ssdn", "gauss25", "known", 3)
    data = batch("ssdn", "gauss25", 3, 4, 32, seed=3)
    clean = data[2][NoisyDataset.Metadata.CLEAN].to(DEV)
    opt = torch.optim.Adam(d.parameters(), lr=3e-4, betas=(0.9, 0.99))
    losses = []
    for _ in range(20):
        opt.zero_grad()
        out = d.run_pipeline(data)
        loss = ((out[PO.IMG_DENOISED] - clean) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("posterior-mean MSE over 20 Adam steps: %.5f -> %.5f" % (losses[0], losses[-1]))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses


# measured on MI355X at the three probe samples: rel-L2 1.7e-5, max |diff| / max |ref| 8.3e-5 (the seeded network's own outputs hold
# pixels with Sx closer to singular than the teacher-forced inputs).  Bounds: 1.5x.
FULL_REL, FULL_ATOL = 2.6e-5, 1.25e-4


# ---- 7. full size -----------------------------------------------------------------------------------------------------------------------
def test_full_size_vjp_all_terms_matches_teacher_forced_probes():
    from ssdn.params import PipelineOutput as PO
    B, Psz, ch = 32, 64, 3
    d = seeded_denoiser("ssdn", "gauss25", "known", ch)
    data = batch("ssdn", "gauss25", ch, B, Psz, seed=7)
    w, gp, gm = upstream(B, ch, Psz, seed=31)
    w, gp, gm = w.to(DEV), gp.to(DEV) * 1e-2, gm.to(DEV) * 1e-2
    out = d.run_pipeline(data)
    L = (out[PO.LOSS].view(B) * w).sum() + (out[PO.IMG_DENOISED] * gp).sum() + (out[PO.IMG_MU] * gm).sum()
    L.backward()
    torch.cuda.synchronize()
    eng = d._last_train_engine
    assert torch.isfinite(d.flat_grad).all() and float(d.flat_grad.abs().max()) > 0
    g32 = eng.main.tensor("g32").cpu()
    net_out, noisy = eng.main.tensor("out32").cpu(), eng.inp.cpu()
    probe = [0, 13, B - 1]
    npar = torch.full((len(probe),), NPAR["gauss25"])
    g64, _ = head_vjp64(net_out[probe], noisy[probe], npar, "gauss25", "known", None, w.cpu()[probe], gp.cpu()[probe], gm.cpu()[probe])
    a, b = g32[probe].double(), g64
    rel = float((a - b).norm() / b.norm())
    print("full size: g_net_out at %d probe samples vs fp64: rel-L2 %.3e, max |diff| / max |ref| %.3e" % (
        len(probe), rel, float((a - b).abs().max() / b.abs().max())))
    assert rel <= FULL_REL
    _cmp(a, b, 2e-4, FULL_ATOL)
