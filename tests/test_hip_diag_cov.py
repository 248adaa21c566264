"""GPU: DIAGONAL_COVARIANCE -- k_head<true> and k_head_vjp<GY, true> teacher-forced against float64 autograd of
the oracle's full head on the scattered output (tests/test_diag_cov_cpu.py), the Denoiser end to end (x.grad, mean(LOSS) bit-identity,
a 3-step Adam trajectory next to an oracle loop, evaluation at a non-training size, a `.wt` round trip, a plan blob through the C ABI
alone), and mono: the same model with or without the flag, bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import restate as R
from test_diag_cov_cpu import CASES, NPAR, diag_cfg, diag_head64, diag_inputs, oracle_diag, scatter9
from test_hip_denoiser import _cat_state, _flat_grad_of, _flat_of
from test_hip_denoiser_autograd import DEV, P, _cos_rel, batch
from head_ops import head_op, head_vjp_op

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def diag_denoiser(style="gauss25", mode="known", ch=3, diag=True, seeded=True):
    """a Denoiser of the diagonal model on the GPU; seeded: the main network from R.make_params(ch, 2*ch, True, seed=5), the sigma network
    (var) from seed 6, a learnt constant (const) at 1.7 -- the setting of tests/test_hip_denoiser_autograd.seeded_denoiser"""
    from ssdn.denoiser import Denoiser
    d = Denoiser(diag_cfg(style, mode, ch, diag), device="cuda:0")
    if seeded:
        d.get_model(Denoiser.MODEL, False).load_state_dict(R.reference_state_dict(R.make_params(ch, 2 * ch, True, seed=5)))
        if mode == "var":
            d.get_model(Denoiser.SIGMA_ESTIMATOR, False).load_state_dict(R.reference_state_dict(R.make_params(ch, 1, False, seed=6)))
        if mode == "const":
            with torch.no_grad():
                d.l_params[Denoiser.ESTIMATED_SIGMA].fill_(1.7)
        d.mark_dirty()
    d.train()
    return d


def close(a, b, rtol, atol, what=""):
    b = b.detach().cpu().double().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    np.testing.assert_allclose(a.detach().cpu().double().numpy().reshape(b.shape), b, rtol=rtol, atol=atol, err_msg=what)


# ---- a. the head ops, teacher-forced (tests/test_hip_head.py's tolerances against the float64 oracle) -------------------------------------
@pytest.mark.parametrize("style,mode", CASES)
def test_diag_head_op_vs_float64(style, mode):
    net_out, noisy, npar, raw = diag_inputs(style, mode)
    B, H = net_out.shape[0], net_out.shape[2]
    est_raw = raw.mean(dim=(1, 2, 3)) if mode == "var" else raw
    r = head_op(net_out, noisy, npar, style, mode, est_raw, diag=1)
    o, g, graw, _ = oracle_diag(net_out, noisy, npar, style, mode, raw, w=torch.full((B,), 1.0 / B))
    close(r["loss"], o["loss"].view(B), 2e-5, 1e-6, "loss")
    close(r["mu"], net_out[:, :3], 0, 0, "mu")
    close(r["pme"], o["out"], 2e-5, 5e-6, "pme")
    close(r["model_std"], o["model_std"], 2e-5, 1e-6, "model_std")
    if style.startswith("poisson"):
        close(r["noise_std"], o["noise_std"], 2e-5, 1e-6, "noise_std")
    else:
        close(r["noise_std"][:1] if mode == "const" else r["noise_std"], o["noise_std"].reshape(-1)[:1 if mode == "const" else B], 2e-5, 1e-7)
    close(r["g_net_out"], g, 2e-4, 1e-6 * float(g.abs().max()), "g_net_out")
    if mode == "const":
        close(r["g_est"][:1], graw.reshape(1), 2e-4, 1e-9, "g_est")
    if mode == "var":
        close(r["g_sig"], graw, 2e-4, 1e-10, "g_sigma_out")
    m = diag_head64(net_out, noisy, npar, style, mode, est_raw.double() if est_raw is not None else None, w=torch.full((B,), 1.0 / B))
    assert float(np.int32(r["gmax"][0].item()).view(np.float32)) == pytest.approx(float(m["g_net_out"].abs().max()), rel=1e-4)


@pytest.mark.parametrize("style,mode", CASES)
def test_diag_head_vjp_op_vs_float64(style, mode):
    net_out, noisy, npar, raw = diag_inputs(style, mode, seed=1)
    B, H = net_out.shape[0], net_out.shape[2]
    est_raw = raw.mean(dim=(1, 2, 3)) if mode == "var" else raw
    g = torch.Generator().manual_seed(17)
    w, gp, gm = torch.randn(B, generator=g), torch.randn(B, 3, H, H, generator=g), torch.randn(B, 3, H, H, generator=g)
    for terms in ((w, gp, gm), (w, None, None), (None, gp, None), (None, None, gm)):
        r = head_vjp_op(net_out, noisy, npar, style, mode, est_raw, *terms, diag=1)
        _, og, oraw, ody = oracle_diag(net_out, noisy, npar, style, mode, raw, *terms)
        close(r["g_net_out"], og, 2e-4, 2e-6 * float(og.abs().max()), "g_net_out")
        close(r["g_noisy"], ody, 2e-4, 4.1e-6 * float(ody.abs().max()) + 1e-30, "g_noisy")
        if mode == "const":
            close(r["g_est"][:1], oraw.reshape(1), 2e-4, 1e-6 * float(oraw.abs().max()) + 1e-12, "g_est")
        if mode == "var":
            close(r["g_sig"], oraw, 2e-4, 1e-6 * float(oraw.abs().max()) + 1e-12, "g_sigma_out")
    # keep: a sample asking for exactly d mean(LOSS) keeps the forward's g_net_out and partials, bit for bit, and still writes g_noisy
    f = head_op(net_out, noisy, npar, style, mode, est_raw, diag=1)
    r = head_vjp_op(net_out, noisy, npar, style, mode, est_raw, torch.full((B,), 1.0 / B), None, None, diag=1, keep=1, g_init=f["g_net_out"],
                    partial_init=f["partial"])
    assert torch.equal(r["g_net_out"], f["g_net_out"]) and torch.equal(r["partial"], f["partial"])
    _, _, _, ody = oracle_diag(net_out, noisy, npar, style, mode, raw, torch.full((B,), 1.0 / B))
    close(r["g_noisy"], ody, 2e-4, 4.1e-6 * float(ody.abs().max()), "g_noisy (keep)")
    # without keep the same request recomputes what the forward wrote
    r = head_vjp_op(net_out, noisy, npar, style, mode, est_raw, torch.full((B,), 1.0 / B), None, None, diag=1)
    close(r["g_net_out"], f["g_net_out"], 1e-5, 1e-6 * float(f["g_net_out"].abs().max()), "VJP of mean(LOSS) vs the forward's gradient")


def test_diag_head_rejects_other_channel_counts():
    from ssdn.hip import lib as L
    from ssdn.hip.engine import OpList, current_stream
    t = torch.zeros(64, device=DEV)
    a = L.HeadArgs(P(t), P(t), P(t), None, 1, 2, 2, 2, 0, 0, 1, None, None, None, None, P(t), P(t), 1, None, 1)
    with pytest.raises(L.SsdnHipError, match="diag"):
        OpList([("head_ssdn", a)]).run(current_stream())
    v = L.HeadVjpArgs(P(t), P(t), P(t), None, 1, 2, 2, 2, 0, 0, P(t), None, None, 0, 1, P(t), P(t), None, None, None, None)
    v.diag = 1
    with pytest.raises(L.SsdnHipError, match="diag"):
        OpList([("head_vjp", v)]).run(current_stream())
    torch.cuda.synchronize()


# ---- b. the Denoiser -----------------------------------------------------------------------------------------------------------------------
def reference_x_grad_diag(d, style, mode, data, w, gp, gm):
    """x.grad through the model's NoiseNetwork autograd (+ the sigma network's, var) and a float64 host head on the scattered output whose
    noisy image is a leaf of its own"""
    from ssdn.denoiser import Denoiser
    noisy = data[0]
    B = noisy.shape[0]
    xr = noisy.detach().clone().requires_grad_(True)
    out = d.get_model(Denoiser.MODEL, False)(xr)
    y64 = noisy.detach().cpu().double().requires_grad_(True)
    est = None
    if mode == "var":
        est = d.get_model(Denoiser.SIGMA_ESTIMATOR, False)(xr).mean(dim=(2, 3), keepdim=True).cpu().double()
    elif mode == "const":
        est = d.l_params[Denoiser.ESTIMATED_SIGMA].detach().cpu().double()
    npar = torch.full((B, 1, 1, 1), NPAR[style], dtype=torch.float64)
    o = R.ssdn_head(scatter9(out.cpu().double()), y64, npar, style, mode, est)
    L = (o["loss"].view(B) * w.cpu().double()).sum() + (o["out"] * gp.cpu().double()).sum() + (o["out_mu"] * gm.cpu().double()).sum()
    L.backward()
    torch.cuda.synchronize()
    return xr.grad.cpu().double() + y64.grad


@pytest.mark.parametrize("style,mode", [("gauss25", "known"), ("poisson30", "const"), ("gauss25", "var")])
def test_diag_x_grad_vs_network_autograd(style, mode):
    from ssdn.params import PipelineOutput as PO
    B, Psz = 4, 32
    d = diag_denoiser(style, mode)
    data = batch("ssdn", style, 3, B, Psz)
    g = torch.Generator().manual_seed(23)
    w = torch.randn(B, generator=g).to(DEV)
    gp, gm = (torch.randn(B, 3, Psz, Psz, generator=g) * 1e-2).to(DEV), (torch.randn(B, 3, Psz, Psz, generator=g) * 1e-2).to(DEV)
    want = reference_x_grad_diag(d, style, mode, data, w, gp, gm)
    x = data[0].detach().clone().requires_grad_(True)
    res = d.run_pipeline([x] + data[1:])
    ((res[PO.LOSS].view(B) * w).sum() + (res[PO.IMG_DENOISED] * gp).sum() + (res[PO.IMG_MU] * gm).sum()).backward()
    torch.cuda.synchronize()
    got = x.grad.cpu().double()
    cos, rel = _cos_rel(got.reshape(-1), want.reshape(-1))
    print("diag x.grad %s/%s: 1 - cosine %.3e, rel err %.3e" % (style, mode, 1 - cos, rel))
    assert torch.isfinite(got).all()
    assert 1 - cos <= 2.7e-5 and rel <= 9e-3, (cos, rel)            # tests/test_hip_denoiser_input_grad.py's bounds


@pytest.mark.parametrize("style,mode", [("gauss25", "known"), ("poisson30", "const"), ("gauss25", "var")])
def test_diag_mean_loss_backward_is_bit_identical_and_reproducible(style, mode):
    from ssdn.params import PipelineOutput as PO
    d = diag_denoiser(style, mode)
    data = batch("ssdn", style, 3, 4, 32)
    out = d.run_pipeline(data)
    d.backward()
    torch.cuda.synchronize()
    g_ref, loss_ref, pme_ref = d.flat_grad.clone(), out[PO.LOSS].detach().clone(), out[PO.IMG_DENOISED].detach().clone()
    assert torch.isfinite(g_ref).all() and float(g_ref.abs().max()) > 0
    for _ in range(2):                                                # autograd route, twice: bit-identical every time
        d.flat_grad.zero_()
        out = d.run_pipeline(data)
        torch.mean(out[PO.LOSS]).backward()
        torch.cuda.synchronize()
        assert torch.equal(out[PO.LOSS].detach(), loss_ref) and torch.equal(out[PO.IMG_DENOISED].detach(), pme_ref)
        assert torch.equal(d.flat_grad, g_ref), "%d of %d gradient elements differ" % (int((d.flat_grad != g_ref).sum()), g_ref.numel())


class DiagCpuTrainer(R.CpuTrainer):
    """the oracle trainer with the diagonal model: the 6-channel output scattered into the full head"""

    def forward(self, noisy, ref=None, noise_param=None, coords=None):
        out = R.net_forward(self.p, noisy, self.blindspot)
        est_raw = None
        if self.mode == "const":
            est_raw = self.est
        elif self.mode == "var":
            est_raw = R.net_forward(self.ps, noisy, False).mean(dim=(2, 3), keepdim=True)
        r = R.ssdn_head(scatter9(out), noisy, noise_param, self.style, self.mode, est_raw)
        r["net_out"] = out
        return r


@pytest.mark.parametrize("style,mode", [("gauss25", "known"), ("poisson30", "const"), ("gauss25", "var")])
def test_diag_training_trajectory(style, mode):
    """Three Adam steps next to the oracle loop, each from the oracle's current state, with tests/test_hip_denoiser.py::
    test_training_trajectory's weights (R.make_params(3, 6, True, seed=5); sigma network seed 6) and bounds.  A learnt constant starts
    at raw 1.7, as in tests/test_hip_denoiser_autograd.py: from raw 0 (est = softplus(-4)) 60% of these pixels have mu <= 1e-3, the
    diagonal model's loss is 887 (the full model's 40) with sy_c = a_c^2 + 2e-5, and the fp16 / bf16 network arithmetic alone moved the
    parameter gradient's cosine to 0.993 (the head ops are checked against float64 above)."""
    from ssdn.denoiser import Denoiser
    from ssdn.datasets import NoisyDataset
    from ssdn.params import PipelineOutput
    from test_oracle_golden import train_inputs
    d = diag_denoiser(style, mode)
    p0 = R.make_params(3, 6, True, seed=5)
    sp0 = R.make_params(3, 1, False, seed=6) if mode == "var" else None
    tr = DiagCpuTrainer("ssdn", 3, style, mode, params=p0, sigma_params=sp0)
    if tr.est is not None:
        with torch.no_grad():
            tr.est.fill_(1.7)
    nets = [(d.get_model(Denoiser.MODEL, False), 0, tr.p)]
    if sp0 is not None:
        nets.append((d.get_model(Denoiser.SIGMA_ESTIMATOR, False), d._n_main, tr.ps))
    clean, noisy, ref, coords, npar = train_inputs("ssdn", style, 3)
    meta = {NoisyDataset.Metadata.INPUT_NOISE_VALUES: npar, NoisyDataset.Metadata.CLEAN: clean}
    for it in range(3):
        lr = R.trainer_lr((it + 1) * 40, 1000)
        start = _flat_of(d, nets, tr)
        d.flat.copy_(start)
        d.adam_m.copy_(_cat_state(d, nets, tr, tr.m))
        d.adam_v.copy_(_cat_state(d, nets, tr, tr.v))
        d.adam_steps = tr.steps
        d.mark_dirty()
        out = d.run_pipeline([noisy, ref, meta])
        d.backward()
        for t in tr.leaves:
            t.grad = None
        r = tr.forward(noisy, ref, npar, coords)
        r["loss"].mean().backward()
        loss = out[PipelineOutput.LOSS].detach().cpu().numpy()
        np.testing.assert_allclose(loss, r["loss"].detach().numpy(), rtol=1e-2, atol=2e-3, err_msg="loss, iteration %d" % it)
        if it == 0:
            o = out[PipelineOutput.IMG_DENOISED].detach().cpu()
            assert float((o - r["out"].detach()).norm() / r["out"].detach().norm()) <= 1e-2
        gd, gr = d.flat_grad.cpu(), _flat_grad_of(d, nets, tr)
        cos = float((gd * gr).sum() / (gd.norm() * gr.norm() + 1e-30))
        agree = float(((gd > 0) == (gr > 0)).float().mean())
        print("diag %s/%s iteration %d: loss %s (oracle %s), gradient cosine %.5f, sign agreement %.4f"
              % (style, mode, it, loss.reshape(-1).tolist(), r["loss"].detach().reshape(-1).tolist(), cos, agree))
        assert cos >= 0.997 and agree >= 0.97, "iteration %d: gradient cosine %.4f, sign agreement %.4f" % (it, cos, agree)
        d.optimizer_step(lr)
        tr.steps += 1
        with torch.no_grad():
            for t, m, v in zip(tr.leaves, tr.m, tr.v):
                R.adam_step(t, t.grad, m, v, tr.steps, lr)
        torch.cuda.synchronize()
        du, ru = d.flat.cpu() - start, _flat_of(d, nets, tr) - start
        ucos = float((du * ru).sum() / (du.norm() * ru.norm() + 1e-30))
        assert ucos >= 0.95, "iteration %d: Adam update cosine %.4f" % (it, ucos)
        assert float(du.abs().max()) <= lr * 3.5


def test_diag_mono_is_bit_identical_to_mono():
    """C = 1: `--diagonal` changes the run name only -- three training steps, outputs and parameters bit for bit"""
    from ssdn.params import PipelineOutput as PO
    a, b = diag_denoiser("gauss25", "known", ch=1, diag=True), diag_denoiser("gauss25", "known", ch=1, diag=False)
    assert torch.equal(a.flat, b.flat)
    data = batch("ssdn", "gauss25", 1, 4, 32)
    for it in range(3):
        oa, ob = a.train_step(data, lr=3e-4), b.train_step(data, lr=3e-4)
        torch.cuda.synchronize()
        for k in (PO.LOSS, PO.IMG_DENOISED, PO.IMG_MU, PO.MODEL_STD_DEV, PO.NOISE_STD_DEV):
            assert torch.equal(oa[k], ob[k]), (it, k)
        assert torch.equal(a.flat, b.flat), it
    assert a.config_name() == b.config_name() + "-diag"


def test_diag_eval_forward_and_wt_round_trip(tmp_path):
    """Evaluation at 256x256 against the oracle; after training steps, a `.wt` reloads through DenoiserEvaluator with the same outputs"""
    from ssdn.datasets import NoisyDataset
    from ssdn.eval import DenoiserEvaluator
    from ssdn.params import PipelineOutput as PO
    d = diag_denoiser("gauss25", "known")
    p = R.make_params(3, 6, True, seed=5)
    S = 256
    x = R.hash_tensor((1, 3, S, S), 77, 0, 1)
    npar = torch.full((1, 1, 1, 1), 25 / 255.0)
    meta = {NoisyDataset.Metadata.INPUT_NOISE_VALUES: npar}
    d.eval()
    with torch.no_grad():
        out = d.run_pipeline([x, None, meta])
    tr = DiagCpuTrainer("ssdn", 3, "gauss25", "known", params=p)
    with torch.no_grad():
        r = tr.forward(x, None, npar)
    o = out[PO.IMG_DENOISED].cpu()
    rel = float((o - r["out"]).norm() / r["out"].norm())
    rel_mu = float((out[PO.IMG_MU].cpu() - r["out_mu"]).norm() / r["out_mu"].norm())
    print("diag eval 256x256: PME rel err %.3e, mu rel err %.3e" % (rel, rel_mu))
    # end to end the fp16 network's error reaches the posterior mean through the per-channel weights sn / (sx + sn) (test_training_trajectory's
    # 1e-2); the head of this evaluation engine, teacher-forced on the network output it computed, is the float64 oracle's to 2e-5
    assert rel_mu <= 5e-3 and rel <= 1e-2, (rel_mu, rel)
    eng = d._last_engine
    t, _, _, _ = oracle_diag(eng.main.tensor("out32").cpu(), x, npar.view(1), "gauss25", "known", None, w=torch.ones(1))
    close(eng.pme, t["out"], 2e-5, 5e-6, "eval PME, teacher-forced")
    close(eng.model_std, t["model_std"], 2e-5, 1e-6, "eval model std, teacher-forced")
    clean = R.hash_tensor((1, 3, S, S), 78, 0, 1)
    assert abs(float(R.psnr(o, clean) - R.psnr(r["out"], clean))) <= 0.05
    # train a few steps, write the model-only checkpoint, reload it as the evaluator does
    d.train()
    data = batch("ssdn", "gauss25", 3, 4, 32)
    for _ in range(3):
        d.train_step(data, lr=3e-4)
    d.eval()
    with torch.no_grad():
        want = d.run_pipeline([x, None, meta])
    sd = {k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in d.state_dict().items()}
    torch.save(sd, tmp_path / "model.wt")
    ev = DenoiserEvaluator(str(tmp_path / "model.wt"), runs_dir=str(tmp_path / "runs"))
    assert ev.denoiser.config_name().endswith("-diag")
    ev.denoiser.eval()
    with torch.no_grad():
        got = ev.denoiser.run_pipeline([x, None, meta])
    for k in (PO.IMG_DENOISED, PO.IMG_MU, PO.MODEL_STD_DEV):
        assert torch.equal(got[k], want[k]), k


def test_diag_plan_blob_through_the_c_abi_alone_is_bit_identical(tmp_path):
    """config 2's shape (ssdn gauss25 sigma_known, batch 32, 64x64) with the diagonal head: the exported blob, run by the unchanged
    tests/plan_c_driver.py in a separate process, gives the Python engine's losses, parameters and posterior mean bit for bit"""
    import fullsize as F
    from ssdn.datasets import NoisyDataset
    from ssdn.hip import lib as L
    from ssdn.params import PipelineOutput
    clean, noisy, npar = F.inputs("cfg2")
    meta = {NoisyDataset.Metadata.INPUT_NOISE_VALUES: npar, NoisyDataset.Metadata.CLEAN: clean}
    torch.manual_seed(21)
    d = diag_denoiser("gauss25", "known", seeded=False)
    params0 = d.flat.detach().cpu().clone()
    lr, steps = 3e-4, 2
    losses = []
    for _ in range(steps):
        out = d.train_step([noisy, clean, meta], lr)
        torch.cuda.synchronize()
        losses.append(out[PipelineOutput.LOSS].detach().cpu().reshape(-1).clone())
    eng = d._last_train_engine
    blob = eng.export_plan(dict(config="config 2, diagonal covariance"))
    (tmp_path / "plan.bin").write_bytes(blob)
    torch.save(dict(params=params0, noisy=noisy, noise_param=npar.reshape(-1), ref=None, coords=None, lr=lr, steps=steps), tmp_path / "in.pt")
    env = dict(os.environ)
    env.pop("PYTHONPATH", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "plan_c_driver.py"), L.LIB_PATH, str(tmp_path / "plan.bin"),
                        str(tmp_path / "in.pt"), str(tmp_path / "out.pt")], capture_output=True, text=True, timeout=600, cwd=str(tmp_path), env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    got = torch.load(tmp_path / "out.pt")
    assert got["meta"]["diag"] is True and got["meta"]["pipeline"] == "ssdn"
    assert [l["M"] for l in got["meta"]["layers"] if l["name"] == "output_block.4"] == [6]
    for a, b in zip(losses, got["loss"]):
        assert torch.equal(a, b.reshape(-1)), (a[:4], b.reshape(-1)[:4])
    n = d.flat.numel()
    assert torch.equal(d.flat.detach().cpu(), got["params"][:n]), "parameters after two steps through the C ABI differ"
    assert torch.equal(eng.pme.cpu().reshape(-1), got["pme"])
