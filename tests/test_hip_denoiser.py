"""GPU: the drop-in `Denoiser` façade end to end (run_pipeline -> backward -> fused Adam) against
(a) the golden training trajectories generated from the reference (tests/golden/g_train_*.npz) and
(b) the oracle trainer run side by side on the host (full tensors), step by step from identical states."""
import os

import numpy as np
import pytest
import torch

import restate as R
from test_oracle_golden import TRAIN_CASES, train_inputs

pytestmark = pytest.mark.gpu


def make_denoiser(alg, style, mode, ch):
    import ssdn
    from ssdn.denoiser import Denoiser
    from ssdn.params import ConfigValue, NoiseAlgorithm, NoiseValue
    cfg = ssdn.cfg.base()
    cfg[ConfigValue.ALGORITHM] = NoiseAlgorithm(alg)
    cfg[ConfigValue.NOISE_STYLE] = style
    cfg[ConfigValue.NOISE_VALUE] = NoiseValue(mode)
    cfg[ConfigValue.IMAGE_CHANNELS] = ch
    ssdn.cfg.infer(cfg, model_only=True)
    return Denoiser(cfg, device="cuda:0")


def _flat_of(d, net_list, tr):
    """oracle trainer state -> the Denoiser's flat parameter layout"""
    f = torch.zeros(d.flat.numel())
    for net, base, cur in net_list:
        for l in net.layers:
            f[base + l.w_off: base + l.w_off + l.M * l.cin * l.k * l.k] = cur[l.name + ".weight"].detach().reshape(-1)
            f[base + l.b_off: base + l.b_off + l.M] = cur[l.name + ".bias"].detach()
    if tr.est is not None:
        f[d._n_main + d._n_sig] = float(tr.est.detach().reshape(-1)[0])
    return f


def _flat_grad_of(d, net_list, tr):
    f = torch.zeros(d.flat.numel())
    for net, base, cur in net_list:
        for l in net.layers:
            f[base + l.w_off: base + l.w_off + l.M * l.cin * l.k * l.k] = cur[l.name + ".weight"].grad.reshape(-1)
            f[base + l.b_off: base + l.b_off + l.M] = cur[l.name + ".bias"].grad
    if tr.est is not None:
        f[d._n_main + d._n_sig] = float(tr.est.grad.reshape(-1)[0])
    return f


@pytest.mark.parametrize("tag,alg,style,mode,ch", TRAIN_CASES)
def test_training_trajectory(golden_dir, tag, alg, style, mode, ch):
    """Three optimisation steps next to the oracle trainer (which tests/test_oracle_golden pins to the reference's
    trajectory fixtures g_train_*).  Every step is checked from the SAME starting point -- the oracle's current weights
    are loaded into the device first -- because these fixtures sit in a very steep part of the loss surface (the loss
    halves per 1e-4 step; measured: a 2.5% sign disagreement on near-zero gradient elements changes the next loss by
    12% for poisson/const), so a free-running comparison would test chaos, not kernels.  Per step:
      loss            1e-2 relative (vs oracle AND vs the reference's golden value)
      gradient        cosine >= 0.985, sign agreement >= 0.95 over all 1.27M (+1.1M) parameters
      Adam update     cosine >= 0.9 with the oracle's update, |update| <= lr everywhere."""
    from ssdn.denoiser import Denoiser
    from ssdn.datasets import NoisyDataset
    from ssdn.params import PipelineOutput
    g = np.load(os.path.join(golden_dir, "g_train_%s.npz" % tag))
    bs = alg == "ssdn"
    cout = ch + ch * (ch + 1) // 2 if alg == "ssdn" else ch
    p0 = R.make_params(ch, cout, bs, seed=5)
    sp0 = R.make_params(ch, 1, False, seed=6) if (mode == "var" and alg == "ssdn") else None
    d = make_denoiser(alg, style, mode, ch)
    d.train()
    tr = R.CpuTrainer(alg, ch, style, mode, params={k: v.clone() for k, v in p0.items()},
                      sigma_params={k: v.clone() for k, v in sp0.items()} if sp0 is not None else None)
    nets = [(d.get_model(Denoiser.MODEL, False), 0, tr.p)]
    if sp0 is not None:
        nets.append((d.get_model(Denoiser.SIGMA_ESTIMATOR, False), d._n_main, tr.ps))
    clean, noisy, ref, coords, npar = train_inputs(alg, style, ch)
    MD = NoisyDataset.Metadata
    meta = {MD.INPUT_NOISE_VALUES: npar, MD.CLEAN: clean}
    if alg == "n2v":
        meta[MD.MASK_COORDS] = coords
    for it in range(3):
        lr = R.trainer_lr((it + 1) * 40, 1000)
        start = _flat_of(d, nets, tr)
        d.flat.copy_(start)
        d.adam_m.copy_(_cat_state(d, nets, tr, tr.m))
        d.adam_v.copy_(_cat_state(d, nets, tr, tr.v))
        d.adam_steps = tr.steps
        d.mark_dirty()
        out = d.run_pipeline([noisy, ref, meta])
        d._last_engine.backward()
        for t in tr.leaves:
            t.grad = None
        r = tr.forward(noisy, ref, npar, coords)
        r["loss"].mean().backward()
        loss = out[PipelineOutput.LOSS].detach().cpu().numpy()
        np.testing.assert_allclose(loss, r["loss"].detach().numpy(), rtol=1e-2, atol=2e-3, err_msg="loss, iteration %d" % it)
        np.testing.assert_allclose(loss, g["loss_it%d" % it], rtol=1e-2, atol=2e-3, err_msg="loss vs reference golden, iteration %d" % it)
        if it == 0:
            o = out[PipelineOutput.IMG_DENOISED].detach().cpu()
            # posterior mean vs the reference's: 1e-2 (with an ESTIMATED, still tiny sigma the PME weights amplify fp16 error)
            assert float((o - torch.from_numpy(g["out0"])).norm() / torch.from_numpy(g["out0"]).norm()) <= 1e-2
        gd, gr = d.flat_grad.cpu(), _flat_grad_of(d, nets, tr)
        cos = float((gd * gr).sum() / (gd.norm() * gr.norm() + 1e-30))
        agree = float(((gd > 0) == (gr > 0)).float().mean())
        # (measured over the six configurations, round 5: cosine >= 0.9981, sign agreement >= 0.980, update cosine >= 0.965)
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
        assert float(du.abs().max()) <= lr * 3.5       # |m_hat/sqrt(v_hat)| <= ~3.2 for betas (0.9, 0.99) in the first steps


def _cat_state(d, net_list, tr, state):
    """oracle Adam moment list (ordered like tr.leaves) -> flat layout"""
    f = torch.zeros(d.flat.numel())
    idx = {id(t): s for t, s in zip(tr.leaves, state)}
    for net, base, cur in net_list:
        for l in net.layers:
            f[base + l.w_off: base + l.w_off + l.M * l.cin * l.k * l.k] = idx[id(cur[l.name + ".weight"])].reshape(-1)
            f[base + l.b_off: base + l.b_off + l.M] = idx[id(cur[l.name + ".bias"])]
    if tr.est is not None:
        f[d._n_main + d._n_sig] = float(idx[id(tr.est)].reshape(-1)[0])
    return f


def test_reference_training_idiom_backward_bridge():
    """`torch.mean(outputs[LOSS]).backward()` (train.py:201) drives the HIP backward; `.grad` of the parameters is a view of
    the flat gradient buffer and torch.optim.Adam over denoiser.parameters() works as in the reference."""
    from ssdn.denoiser import Denoiser
    from ssdn.datasets import NoisyDataset
    from ssdn.params import PipelineOutput
    d = make_denoiser("ssdn", "gauss25", "known", 3)
    d.train()
    clean, noisy, ref, coords, npar = train_inputs("ssdn", "gauss25", 3)
    meta = {NoisyDataset.Metadata.INPUT_NOISE_VALUES: npar, NoisyDataset.Metadata.CLEAN: clean}
    opt = torch.optim.Adam(d.parameters(), betas=[0.9, 0.99])
    opt.zero_grad()
    out = d.run_pipeline([noisy, ref, meta])
    torch.mean(out[PipelineOutput.LOSS]).backward()
    w = d.get_model(Denoiser.MODEL, False).get_submodule("decode_block_1.2").weight
    assert w.grad is not None and float(w.grad.abs().sum()) > 0
    assert w.grad.data_ptr() >= d.flat_grad.data_ptr()
    before = w.detach().clone()
    opt.step()
    assert float((w.detach() - before).abs().max()) > 0


def test_external_optimizer_step_refreshes_the_weight_shadows():
    """The reference idiom end to end, twice: after `torch.optim.Adam.step()` on the parameter views the NEXT run_pipeline must
    see the new weights (the fp16/bf16 MFMA shadows are re-packed when the flat buffer's version counter moves) -- and the
    same for NoiseNetwork.forward of the owned model."""
    from ssdn.denoiser import Denoiser
    from ssdn.datasets import NoisyDataset
    from ssdn.params import PipelineOutput
    d = make_denoiser("ssdn", "gauss25", "known", 3)
    d.train()
    clean, noisy, ref, coords, npar = train_inputs("ssdn", "gauss25", 3)
    meta = {NoisyDataset.Metadata.INPUT_NOISE_VALUES: npar, NoisyDataset.Metadata.CLEAN: clean}
    opt = torch.optim.Adam(d.parameters(), lr=2e-5, betas=[0.9, 0.99])     # (these fixtures sit on a very steep loss surface)
    net = d.get_model(Denoiser.MODEL, False)
    losses, outs = [], []
    for _ in range(3):
        opt.zero_grad()
        out = d.run_pipeline([noisy, ref, meta])
        outs.append(net(noisy.to("cuda:0")).cpu())
        torch.mean(out[PipelineOutput.LOSS]).backward()
        losses.append(float(out[PipelineOutput.LOSS].mean()))
        opt.step()
    assert losses[0] != losses[1] and losses[1] != losses[2], losses
    assert losses[2] < losses[0], losses                          # and it actually descends
    assert not torch.equal(outs[0], outs[1])                      # NoiseNetwork.forward sees the update too
    # the fused path afterwards: train_step changes the next loss as well
    d.train_step([noisy, ref, meta], lr=2e-5)
    before = float(d.run_pipeline([noisy, ref, meta])[PipelineOutput.LOSS].mean())
    d.train_step([noisy, ref, meta], lr=2e-5)
    assert float(d.run_pipeline([noisy, ref, meta])[PipelineOutput.LOSS].mean()) != before


def test_loss_backward_uses_its_own_engine_and_outputs_are_fresh_tensors():
    """An eval / differently shaped run_pipeline between a training forward and `.backward()` must not disturb it (the LOSS
    carries the engine that produced it), and results of one call survive the next call (fresh tensors, like the reference)."""
    from ssdn.datasets import NoisyDataset
    from ssdn.params import PipelineOutput
    d = make_denoiser("ssdn", "gauss25", "known", 3)
    clean, noisy, ref, coords, npar = train_inputs("ssdn", "gauss25", 3)
    meta = {NoisyDataset.Metadata.INPUT_NOISE_VALUES: npar, NoisyDataset.Metadata.CLEAN: clean}
    d.train()
    out = d.run_pipeline([noisy, ref, meta])
    d.backward()
    torch.cuda.synchronize()
    g_ref = d.flat_grad.clone()
    d.flat_grad.zero_()
    out = d.run_pipeline([noisy, ref, meta])
    kept = out[PipelineOutput.IMG_DENOISED]
    kept_copy = kept.clone()
    d.eval()
    with torch.no_grad():
        other = d.run_pipeline([noisy[:1].flip(2), None, {NoisyDataset.Metadata.INPUT_NOISE_VALUES: npar[:1]}])   # another engine
        same_shape = d.run_pipeline([noisy * 0.5, None, meta])                                                      # and an eval one of the same shape
    d.train()
    torch.mean(out[PipelineOutput.LOSS]).backward()
    torch.cuda.synchronize()
    assert torch.equal(d.flat_grad, g_ref)
    assert torch.equal(kept, kept_copy) and not torch.equal(kept, same_shape[PipelineOutput.IMG_DENOISED])
    d.optimizer_step(1e-4)            # acts on the training engine although eval engines ran last


def test_optimizer_state_dict_round_trip_in_reference_layout():
    """`.training` checkpoints carry torch.optim.Adam.state_dict() (train.py:725): export after fused steps, load into a real
    torch.optim.Adam over denoiser.parameters(), and back into a fresh Denoiser."""
    from ssdn.datasets import NoisyDataset
    d = make_denoiser("ssdn", "gauss25", "const", 3)
    d.train()
    clean, noisy, ref, coords, npar = train_inputs("ssdn", "gauss25", 3)
    meta = {NoisyDataset.Metadata.INPUT_NOISE_VALUES: npar, NoisyDataset.Metadata.CLEAN: clean}
    for _ in range(2):
        d.train_step([noisy, ref, meta], lr=1e-4)
    sd = d.optimizer_state_dict(lr=1e-4)
    params = list(d.parameters())
    assert len(sd["state"]) == len(params) == len(sd["param_groups"][0]["params"])
    opt = torch.optim.Adam(d.parameters(), lr=1e-4, betas=[0.9, 0.99])
    opt.load_state_dict(sd)                                                    # the layout torch expects
    for i, p in enumerate(params):
        assert opt.state[p]["exp_avg"].shape == p.shape and float(opt.state[p]["step"]) == 2.0
    d2 = make_denoiser("ssdn", "gauss25", "const", 3)
    d2.load_state_dict(d.state_dict())
    d2.load_optimizer_state_dict(opt.state_dict())
    assert d2.adam_steps == 2 and torch.equal(d2.adam_m, d.adam_m) and torch.equal(d2.adam_v, d.adam_v)
    d.train_step([noisy, ref, meta], lr=1e-4)
    d2.train()
    d2.train_step([noisy, ref, meta], lr=1e-4)
    torch.cuda.synchronize()
    assert torch.equal(d.flat, d2.flat)                                       # resumed run == uninterrupted run, bit for bit


def test_backward_with_bucket_events_is_bit_identical():
    """Data parallel step driver on one GPU: the backward list that carries the bucket event records (what the RCCL stream
    waits on) produces bit-identical gradients to the plain list, and every bucket's event completes."""
    from ssdn.datasets import NoisyDataset
    from ssdn.hip import dp
    from ssdn.denoiser import Denoiser
    d = make_denoiser("ssdn", "gauss25", "var", 3)
    d.train()
    clean, noisy, ref, coords, npar = train_inputs("ssdn", "gauss25", 3)
    meta = {NoisyDataset.Metadata.INPUT_NOISE_VALUES: npar, NoisyDataset.Metadata.CLEAN: clean}
    d._run([noisy, ref, meta], clone=False)
    eng = d._last_train_engine
    eng.backward()
    torch.cuda.synchronize()
    g_plain = d.flat_grad.clone()
    d.flat_grad.fill_(float("nan"))
    net = d.get_model(Denoiser.MODEL, False)
    ex = dp.GradExchange(1, dp.bucket_ranges(net.layers, d._n_main, d.flat.numel()), d.device, force_events=True)
    assert ex.overlapped and len(ex.ranges) == 5
    d._run([noisy, ref, meta], clone=False)
    scale = dp.exchange_step(lambda e: eng.backward(exchange=e), d.flat_grad, ex)
    torch.cuda.synchronize()
    assert scale == 1.0 and all(e.query() for e in ex.events)
    n = d._n_main + d._n_sig                      # (the buffer is padded to a multiple of 4; padding is never written)
    assert torch.equal(d.flat_grad[:n], g_plain[:n])
    # ranges cover the buffer exactly once
    cov = torch.zeros(d.flat.numel())
    for lo, hi in ex.ranges:
        cov[lo:hi] += 1
    assert bool((cov[:d._n_main + d._n_sig] == 1).all())


def test_eval_forward_any_square_size():
    """Inference at a non-training size (eval pads Kodak to 768x768, BSD300 to 512x512; here 96x96 to stay small):
    Denoiser.forward == IMG_DENOISED of the pipeline, vs the oracle."""
    from ssdn.denoiser import Denoiser
    d = make_denoiser("ssdn", "gauss25", "known", 3)
    p = R.make_params(3, 9, True, seed=5)
    d.get_model(Denoiser.MODEL, False).load_state_dict(R.reference_state_dict(p))
    d.mark_dirty()
    d.eval()
    from ssdn.datasets import NoisyDataset
    from ssdn.params import PipelineOutput
    x = R.hash_tensor((1, 3, 96, 96), 77, 0, 1)
    meta = {NoisyDataset.Metadata.INPUT_NOISE_VALUES: torch.full((1, 1, 1, 1), 25 / 255.0)}
    with torch.no_grad():
        out = d.run_pipeline([x, None, meta])
    tr = R.CpuTrainer("ssdn", 3, "gauss25", "known", params=p)
    with torch.no_grad():
        r = tr.forward(x, None, torch.full((1, 1, 1, 1), 25 / 255.0))
    o = out[PipelineOutput.IMG_DENOISED].cpu()
    assert float((o - r["out"]).norm() / r["out"].norm()) <= 5e-3
    # PSNR criterion of BASELINE.json: same weights => within 0.05 dB of the reference path
    clean = R.hash_tensor((1, 3, 96, 96), 78, 0, 1)
    assert abs(float(R.psnr(o, clean) - R.psnr(r["out"], clean))) <= 0.05


@pytest.mark.parametrize("transpose,shape", [(False, (50, 90)), (True, (90, 50))])
def test_eval_forward_non_square_size(transpose, shape):
    """Validation of a plain-network run (N2C here; ssdn/train.py pads such a validation set to multiples of 32 per side, not to squares: BSD
    at 352x512 / 512x352, Kodak at 512x768 / 768x512, batch 1; here 64x96 and its transpose 96x64 to stay small, ragged tiles down to a 2x3
    stage): IMG_DENOISED against the oracle, the device's per-sample PSNR over the un-padded extent (also non-square) against the host
    formula on the device's own output, and the PSNR criterion of BASELINE.json against the oracle path.
    Measured: relative L2 8.1e-4 (64x96) and 7.7e-4 (96x64), PSNR within 2e-3 dB of the oracle path, device PSNR equal to the host's to 1e-6."""
    from ssdn.denoiser import Denoiser
    from ssdn.datasets import NoisyDataset
    from ssdn.params import PipelineOutput
    MD = NoisyDataset.Metadata
    d = make_denoiser("n2c", "gauss25", "known", 3)
    p = R.make_params(3, 3, False, seed=5)
    d.get_model(Denoiser.MODEL, False).load_state_dict(R.reference_state_dict(p))
    d.mark_dirty()
    d.eval()
    x, clean = R.hash_tensor((1, 3, 64, 96), 77, 0, 1), R.hash_tensor((1, 3, 64, 96), 78, 0, 1)
    if transpose:
        x, clean = x.transpose(2, 3).contiguous(), clean.transpose(2, 3).contiguous()
    e1, e2 = shape
    data = [x, None, {MD.INPUT_NOISE_VALUES: torch.full((1, 1, 1, 1), 25 / 255.0), MD.CLEAN: clean, MD.IMAGE_SHAPE: torch.tensor([[3, e1, e2]])}]
    with torch.no_grad():
        out = d.run_pipeline(data)
        per = d.accumulate_metrics(data, "valid", with_loss=False, per_sample=True)
    o = out[PipelineOutput.IMG_DENOISED].cpu()
    assert tuple(o.shape) == tuple(x.shape)
    tr = R.CpuTrainer("n2c", 3, "gauss25", "known", params=p)
    with torch.no_grad():
        r = tr.forward(x, None, None)
    rel = float((o - r["out"]).norm() / r["out"].norm())
    want = float(-10 * torch.log10(((o[:, :, :e1, :e2].double() - clean[:, :, :e1, :e2].double()) ** 2).mean()))
    dpsnr = abs(float(R.psnr(o, clean) - R.psnr(r["out"], clean)))
    print("%s: rel %.3e, device PSNR %.6f host %.6f, PSNR difference to the oracle path %.2e dB" % (tuple(x.shape), rel, float(per["psnr_out"][0]), want, dpsnr))
    assert rel <= 5e-3
    np.testing.assert_allclose(per["psnr_out"].numpy(), [want], rtol=2e-5)
    # PSNR criterion of BASELINE.json: same weights => within 0.05 dB of the reference path
    assert dpsnr <= 0.05


def _n2v_step_inputs(B, H, W):
    """a Noise2Void minibatch at H != W: one masked pixel per 8x8 box, (row, col) as include/ssdn_hip.h documents ssdn_mse_args.coords --
    half of the columns are >= H, so a swapped lookup leaves the plane"""
    clean = R.hash_tensor((B, 3, H, W), 61, 0, 1)
    noisy = torch.clamp(clean + R.hash_tensor((B, 3, H, W), 62, -1, 1) * 0.17, 0, 1)
    ref = torch.clamp(clean + R.hash_tensor((B, 3, H, W), 63, -1, 1) * 0.17, 0, 1)
    ii, jj = torch.meshgrid(torch.arange(H // 8), torch.arange(W // 8), indexing="ij")
    inside = R.hash_tensor((B, (H // 8) * (W // 8), 2), 64, 0, 8).long().clamp(0, 7)
    coords = torch.stack([ii.reshape(-1) * 8, jj.reshape(-1) * 8], 1)[None] + inside
    return clean, noisy, ref, coords


def test_n2v_training_step_non_square():
    """One Noise2Void step at B = 2, 32x64 (BASELINE config 4's algorithm; k_conv_thin's smallest non-square image) next to the oracle
    trainer from the same weights: the masked loss at test_training_trajectory's tolerance, every parameter tensor's gradient within the
    bounds of tests/test_hip_ops.py::test_net_backward_end_to_end against the fp32 oracle (relative L2 <= 0.13, cosine >= 0.995).
    Measured: loss within 2.4e-4 relative; worst parameter tensor relative L2 0.026, cosine 0.99968 (the fp16 CPU interpreter: 0.022, 0.99977)."""
    from ssdn.denoiser import Denoiser
    from ssdn.datasets import NoisyDataset
    from ssdn.params import PipelineOutput
    MD = NoisyDataset.Metadata
    B, H, W = 2, 32, 64
    clean, noisy, ref, coords = _n2v_step_inputs(B, H, W)
    assert int(coords[0, :, 0].max()) < H and int((coords[0, :, 1] >= H).sum()) >= 8
    p0 = R.make_params(3, 3, False, seed=5)
    d = make_denoiser("n2v", "gauss25", "known", 3)
    d.train()
    tr = R.CpuTrainer("n2v", 3, "gauss25", "known", params={k: v.clone() for k, v in p0.items()})
    net = d.get_model(Denoiser.MODEL, False)
    nets = [(net, 0, tr.p)]
    d.flat.copy_(_flat_of(d, nets, tr))
    d.mark_dirty()
    out = d.run_pipeline([noisy, ref, {MD.INPUT_NOISE_VALUES: torch.full((B, 1, 1, 1), 25 / 255.0), MD.CLEAN: clean, MD.MASK_COORDS: coords}])
    d._last_engine.backward()
    torch.cuda.synchronize()
    r = tr.forward(noisy, ref, None, coords)
    r["loss"].mean().backward()
    loss = out[PipelineOutput.LOSS].detach().cpu().numpy()
    print("loss %s oracle %s" % (loss.reshape(-1).tolist(), r["loss"].detach().reshape(-1).tolist()))
    np.testing.assert_allclose(loss, r["loss"].detach().numpy(), rtol=1e-2, atol=2e-3)
    o = out[PipelineOutput.IMG_DENOISED].detach().cpu()
    assert float((o - r["out"].detach()).norm() / r["out"].detach().norm()) <= 5e-3
    gd, gr = d.flat_grad.cpu(), _flat_grad_of(d, nets, tr)
    bad, worst = [], [0.0, 1.0]
    for l in net.layers:
        for nm, sl in (("w", slice(l.w_off, l.w_off + l.M * l.cin * l.k * l.k)), ("b", slice(l.b_off, l.b_off + l.M))):
            a, b = gd[sl], gr[sl]
            cos = float((a * b).sum() / (a.norm() * b.norm() + 1e-30))
            rel = float((a - b).norm() / (b.norm() + 1e-30))
            worst = [max(worst[0], rel), min(worst[1], cos)]
            if not (rel <= 0.13 and cos >= 0.995):
                bad.append("%s.%s rel %.3e cos %.5f" % (l.name, nm, rel, cos))
    print("worst parameter tensor vs fp32 oracle: rel %.4e cos %.6f" % tuple(worst))
    assert not bad, bad


def test_gradient_agreement_structured_images():
    """Parameter gradients at identical weights, device (fp16 activations, bf16 gradients) vs the fp32 oracle, on STRUCTURED images
    (smooth textures + gauss25 noise, reference-style He-normal init -- the regime the network trains in).  Measured with
    tools/convergence.py (profiles/r02_convergence.json): per-layer cosine >= 0.99995, relative L2 <= 1.1e-2, sign agreement
    0.998.  (The hash-noise fixtures of test_training_trajectory are the adversarial case: LeakyReLU branches of near-zero
    activations flip, hence their looser 0.985 bound.)"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from convergence import textures
    import ssdn
    from ssdn.datasets import NoisyDataset
    from ssdn.denoiser import Denoiser
    from ssdn.params import ConfigValue, NoiseAlgorithm, NoiseValue
    B, P = 4, 64
    cfg = ssdn.cfg.base()
    cfg[ConfigValue.ALGORITHM] = NoiseAlgorithm.SELFSUPERVISED_DENOISING
    cfg[ConfigValue.NOISE_STYLE] = "gauss25"
    cfg[ConfigValue.NOISE_VALUE] = NoiseValue.KNOWN
    ssdn.cfg.infer(cfg, model_only=True)
    torch.manual_seed(0)
    d = Denoiser(cfg, device="cuda:0")
    net = d.get_model(Denoiser.MODEL, False)
    p0 = {k.replace("output_conv", "output_block.4"): v.detach().cpu().clone() for k, v in net.state_dict().items() if not k.startswith("output_conv")}
    tr = R.CpuTrainer("ssdn", 3, "gauss25", "known", params={k: v.clone() for k, v in p0.items()})
    nets = [(net, 0, tr.p)]
    sigma = 25 / 255.0
    clean = textures(B, P, 4242)
    noisy = (clean + torch.randn(clean.shape, generator=torch.Generator().manual_seed(7)) * sigma).clamp(0, 1)
    npar = torch.full((B, 1, 1, 1), sigma)
    MD = NoisyDataset.Metadata
    d.train()
    d.run_pipeline([noisy, None, {MD.INPUT_NOISE_VALUES: npar, MD.CLEAN: clean}])
    d.backward()
    torch.cuda.synchronize()
    r = tr.forward(noisy, None, npar)
    r["loss"].mean().backward()
    gd, gr = d.flat_grad.cpu(), _flat_grad_of(d, nets, tr)
    worst = []
    for l in net.layers:
        sl = slice(l.w_off, l.w_off + l.M * l.cin * l.k * l.k)
        a, b = gd[sl], gr[sl]
        cos = float((a * b).sum() / (a.norm() * b.norm() + 1e-30))
        rel = float((a - b).norm() / (b.norm() + 1e-30))
        if not (cos >= 0.9995 and rel <= 3e-2):
            worst.append("%s cos %.5f rel %.3e" % (l.name, cos, rel))
    assert not worst, worst
    n = d._n_main
    assert float(((gd[:n] > 0) == (gr[:n] > 0)).float().mean()) >= 0.99


@pytest.mark.parametrize("alg,style,mode", [("ssdn", "gauss25", "known"), ("ssdn", "gauss25", "var"), ("ssdn", "poisson30", "const"), ("n2v", "gauss25", "known")])
def test_fused_adam_repack_is_bit_identical_to_adam_then_wpack(alg, style, mode):
    """The optimiser list is [SSDN_OP_ADAM, SSDN_OP_WPACK x layers] per network; the executor runs it as ONE launch (k_adam_pack: the
    thread that updates a weight writes its fp16 / bf16 shadows).  The parameters, the moments and EVERY shadow (forward, data
    gradient, and their chunk-major copies) must equal, bit for bit, what the plain Adam launch followed by the re-pack produces."""
    import ctypes as C
    from ssdn.hip import lib as L
    from ssdn.hip.engine import OpList, current_stream
    d = make_denoiser(alg, style, mode, 3)
    d.train()
    eng = d._engine(2, 32, 32, True)
    g = torch.Generator().manual_seed(3)
    d.flat_grad.copy_(torch.randn(d.flat.numel(), generator=g) * 1e-3)
    start = [t.clone() for t in (d.flat, d.adam_m, d.adam_v)]
    nets = [eng.main] + ([eng.sigma] if eng.sigma is not None else [])
    shadow_names = [(net, k) for net in nets for k in net.t if any(k.startswith(net.plan.prefix + s) for s in ("wf/", "wd/", "wfc/", "wdc/"))]
    assert len(shadow_names) >= 20 * len(nets)

    # fused: the engine's own optimiser list
    eng.adam(3e-4, 1, 0.5)
    torch.cuda.synchronize()
    fused = [t.clone() for t in (d.flat, d.adam_m, d.adam_v)] + [net.t[k].clone() for net, k in shadow_names]
    # reference: the same start, plain SSDN_OP_ADAM over the whole buffer (alone in its list: nothing to fuse), then the re-pack lists
    for t, s0 in zip((d.flat, d.adam_m, d.adam_v), start):
        t.copy_(s0)
    for net, k in shadow_names:
        net.t[k].fill_(0)
    a = L.AdamArgs(d.flat.data_ptr(), d.flat_grad.data_ptr(), d.adam_m.data_ptr(), d.adam_v.data_ptr(), d.flat.numel(),
                   3e-4, 0.9, 0.99, 1e-8, 1.0 - 0.9, 1.0 - 0.99, 0.5)
    OpList([("adam", a)]).run(current_stream())
    eng.repack()
    torch.cuda.synchronize()
    plain = [t.clone() for t in (d.flat, d.adam_m, d.adam_v)] + [net.t[k].clone() for net, k in shadow_names]
    names = ["params", "m", "v"] + [k for _, k in shadow_names]
    for nm, x, y in zip(names, fused, plain):
        assert torch.equal(x.view(torch.uint8) if x.dtype not in (torch.float32,) else x, y.view(torch.uint8) if y.dtype not in (torch.float32,) else y), nm
    assert not torch.equal(fused[0], start[0])                    # (the step did move the parameters)


@pytest.mark.parametrize("alg,style,mode", [("ssdn", "gauss25", "known"), ("ssdn", "poisson30", "const"), ("n2c", "gauss25", "known")])
def test_device_metric_accumulators_equal_the_host_formulas(alg, style, mode):
    """H11: `train_step(metrics=True)` leaves the step's loss / PSNR / std-dev sums in a device accumulator (one SSDN_OP_METRICS launch
    per step); after three steps `read_metrics()` must equal what the reference trainer's per-step lines accumulate on the host
    (train.py:205-218: `Metric += value` with utils/data.py:94-105 and utils/utils.py Metric.add) to 1e-5 relative."""
    import ssdn
    from ssdn.datasets import NoisyDataset
    from ssdn.params import PipelineOutput
    from ssdn.utils import Metric
    MD = NoisyDataset.Metadata
    d = make_denoiser(alg, style, mode, 3)
    d.train()
    B, P = 4, 32
    host = {}
    for step in range(3):
        clean = R.hash_tensor((B, 3, P, P), 500 + step, 0, 1)
        noisy = torch.clamp(clean + R.hash_tensor((B, 3, P, P), 600 + step, -1, 1) * 0.17, 0, 1)
        data = [noisy.cuda(), clean.cuda(), {MD.INPUT_NOISE_VALUES: torch.full((B, 1, 1, 1), 25 / 255.0), MD.CLEAN: clean.cuda(),
                                             MD.IMAGE_SHAPE: torch.tensor([3, P, P]).repeat(B, 1)}]
        out = d.train_step(data, 3e-4, None, metrics=True)
        torch.cuda.synchronize()
        host.setdefault("loss", Metric()).add(out[PipelineOutput.LOSS].detach().cpu().clone())
        host.setdefault("psnr_out", Metric()).add(ssdn.utils.calculate_psnr(out[PipelineOutput.IMG_DENOISED].detach().cpu(), clean))
        if PipelineOutput.IMG_MU in out:
            host.setdefault("psnr_mu_out", Metric()).add(ssdn.utils.calculate_psnr(out[PipelineOutput.IMG_MU].detach().cpu(), clean))
        for key in (PipelineOutput.NOISE_STD_DEV, PipelineOutput.MODEL_STD_DEV):
            if key in out:
                host.setdefault(key.value, Metric()).add(out[key].detach().cpu().clone() * 255)
    got = d.read_metrics("train", reset=True)
    assert set(got) == set(host), (sorted(got), sorted(host))
    for name, m in host.items():
        total, count = got[name]
        assert count == m.n, (name, count, m.n)
        assert float(total) == pytest.approx(float(torch.as_tensor(m.total).sum()), rel=1e-5, abs=1e-6), name
    assert d.read_metrics("train") == {}                       # reset


def test_sigma_network_beside_the_main_network_is_bit_identical():
    """BASELINE config 3 (sigma estimated per image by a second network): the estimator's op lists run on a second stream beside the main
    network's (DenoiserEngine.SIGMA_CONCURRENT, ordered by ssdn_stream_order) -- every step's flat gradient and the parameters after three
    steps are bit-identical to the sequential order's, run after run.  (The first version ordered the streams through torch.cuda.Event /
    ExternalStream: in ~3 of 10 runs the estimator's backward list started before the loss head had written its upstream gradient.)
    Replaces the two sequential nn.Module calls of ssdn/ssdn/denoiser.py:261-265."""
    import torch
    from ssdn.datasets import NoisyDataset
    from ssdn.hip.engine import DenoiserEngine
    B, P, steps = 32, 64, 3
    g = torch.Generator().manual_seed(3)
    clean = torch.rand(B, 3, P, P, generator=g)
    noisy = (clean + torch.randn(B, 3, P, P, generator=g) * 0.1).clamp(0, 1)
    MD = NoisyDataset.Metadata
    saved = DenoiserEngine.SIGMA_CONCURRENT

    def run(mode):
        DenoiserEngine.SIGMA_CONCURRENT = mode
        torch.manual_seed(0)
        d = make_denoiser("ssdn", "gauss25", "var", 3)
        d.train()
        grads = []
        for _ in range(steps):
            d.train_step([noisy.cuda(), None, {MD.INPUT_NOISE_VALUES: torch.full((B, 1, 1, 1), 0.1), MD.CLEAN: clean.cuda()}], 3e-4)
            torch.cuda.synchronize()
            grads.append(d.flat_grad.clone())
        return d.flat.clone(), grads
    try:
        seq, gseq = run(0)
        for rep in range(6):
            con, gcon = run(3)
            for i in range(steps):
                assert torch.equal(gseq[i], gcon[i]), "run %d, step %d: %d gradient elements differ" % (rep, i, int((gseq[i] != gcon[i]).sum()))
            assert torch.equal(seq, con)
    finally:
        DenoiserEngine.SIGMA_CONCURRENT = saved
