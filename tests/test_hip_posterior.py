"""GPU: SSDN_OP_HEAD_POSTERIOR (csrc/head_posterior.hip) against the float64 mirror (tests/posterior_ref.py), its output subsets, the
determinism and the statistics of its samples, Denoiser.posterior and `ssdn eval --posterior`."""
import csv
import math
import os

import numpy as np
import pytest
import torch

import restate as R
from posterior_ops import posterior_op
from posterior_ref import fp32_yardstick, full_matrix, is_impulse, op_inputs, posterior_ref
from test_hip_denoiser_autograd import DEV
from test_impulse_cpu import impulse_cfg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (style, mode, C, diag, alpha)
OP_CASES = [(s, m, C, 0, None) for s in ("gauss25", "poisson30") for m in ("known", "const", "var") for C in (1, 3)]
OP_CASES += [(s, m, 3, 1, None) for s in ("gauss25", "poisson30") for m in ("known", "const", "var")]
OP_CASES += [("impulse", m, C, 0, a) for m in ("known", "const", "var") for C in (1, 3) for a in (0.05, 0.5)]


def close(a, b, rtol, atol, what=""):
    b = b.detach().cpu().double().numpy()
    np.testing.assert_allclose(a.detach().cpu().double().numpy().reshape(b.shape), b, rtol=rtol, atol=atol, err_msg=what)


def _atol(start, fig):
    """the starting tolerance, widened to at most 4x the fp32 mirror's own error on the same inputs (test_hip_impulse.py's rule)"""
    return max(start, 4 * fig)


def _check_op(style, mode, C, diag, alpha, H, W, nchunks):
    no, y, npar, est = op_inputs(style, mode, C, diag, H=H, W=W, alpha=alpha or 0.5)
    m = posterior_ref(no, y, npar, style, mode, est, diag)
    fig = fp32_yardstick(no, y, npar, style, mode, est, diag, m)
    r = posterior_op(no, y, npar, style, mode, est, diag=diag, nchunks=nchunks)
    a_cov = _atol(1e-6 * float(m["cov"].abs().max()), fig["cov"])
    a_std = _atol(1e-6 * float(m["std"].abs().max()), fig["std"])
    print("kernel vs float64: cov %.3e (atol %.3e), std %.3e (atol %.3e)" % (
        float((r["cov"].cpu().double() - m["cov"]).abs().max()), a_cov, float((r["std"].cpu().double() - m["std"]).abs().max()), a_std))
    close(r["cov"], m["cov"], 2e-5, a_cov, "cov")
    close(r["std"], m["std"], 2e-5, a_std, "std")
    assert torch.isnan(r["samples"]).all()                      # not requested: untouched
    ev = torch.linalg.eigvalsh(full_matrix(r["cov"].cpu().double()))
    print("smallest eigenvalue %.3e" % float(ev.min()))
    assert float(ev.min()) >= -a_cov
    return no, y, npar, est, r


@pytest.mark.parametrize("style,mode,C,diag,alpha", OP_CASES)
def test_posterior_op_vs_float64(style, mode, C, diag, alpha):
    """B 2, 5x7, two uneven chunks of less than a workgroup"""
    _check_op(style, mode, C, diag, alpha, 5, 7, 2)


@pytest.mark.parametrize("style,mode,C,diag,alpha", [("gauss25", "known", 3, 0, None)])
def test_posterior_op_vs_float64_several_blocks(style, mode, C, diag, alpha):
    """32x32 in three chunks (342, 342, 340 pixels: more than one pass of a workgroup's 256 threads)"""
    no, y, npar, est, r = _check_op(style, mode, C, diag, alpha, 32, 32, 3)
    r1 = posterior_op(no, y, npar, style, mode, est, diag=diag, nchunks=1)
    assert torch.equal(r1["cov"], r["cov"]) and torch.equal(r1["std"], r["std"])


@pytest.mark.parametrize("style,C,diag", [("gauss25", 3, 0), ("poisson30", 3, 1), ("gauss25", 1, 0), ("impulse", 3, 0), ("impulse", 1, 0)])
def test_output_subsets_give_the_same_bits(style, C, diag):
    no, y, npar, est = op_inputs(style, "const", C, diag, H=5, W=7)
    kw = dict(diag=diag, n_samples=3, seed=11, offset=5)
    full = posterior_op(no, y, npar, style, "const", est, **kw)
    assert all(torch.isfinite(full[k]).all() for k in ("cov", "std", "samples"))
    for only in ("cov", "std", "samples"):
        r = posterior_op(no, y, npar, style, "const", est, want=(only,), **kw)
        assert torch.equal(r[only], full[only]), only
        for other in {"cov", "std", "samples"} - {only}:
            assert torch.isnan(r[other]).all(), (only, other)


@pytest.mark.parametrize("style,C,diag", [("gauss25", 3, 0), ("gauss25", 3, 1), ("poisson30", 1, 0), ("impulse", 3, 0), ("impulse", 1, 0)])
def test_samples_are_a_pure_function_of_seed_offset_index_and_pixel(style, C, diag):
    no, y, npar, est = op_inputs(style, "known", C, diag, H=32, W=32)
    run = lambda **kw: posterior_op(no, y, npar, style, "known", est, diag=diag, want=("samples",),       # noqa: E731
                                    **{**dict(n_samples=16, seed=3, offset=9, nchunks=1), **kw})["samples"]
    a = run()
    assert torch.isfinite(a).all() and torch.equal(a, run())
    assert not torch.equal(a, run(offset=10)) and not torch.equal(a, run(seed=4)) and not torch.equal(a, run(seed=3 + (1 << 32)))
    assert not torch.equal(a[0], a[1]) and not torch.equal(a[:, 0], a[:, 1])                # samples and batch elements differ
    assert torch.equal(run(n_samples=64)[:16], a)
    assert torch.equal(run(nchunks=3), a)


def _moment_bounds(x, mean, cov, S, what):
    """x [S, N, C] samples, mean [N, C], cov [N, C, C] (float64): the sample mean within 6 sqrt(S_ii / S) and the sample covariance within
    6 sqrt((S_ii S_jj + S_ij^2) / (S - 1)) of them, per element (the standard errors of Gaussian samples)"""
    sm = x.mean(0)
    dg = torch.diagonal(cov, dim1=-2, dim2=-1)
    se_m = (dg / S).sqrt()
    zm = ((sm - mean).abs() / se_m.clamp(min=1e-30)).max()
    xc = x - sm
    sc = torch.einsum("sni,snj->nij", xc, xc) / (S - 1)
    se_c = ((dg[:, :, None] * dg[:, None, :] + cov * cov) / (S - 1)).sqrt()
    zc = ((sc - cov).abs() / se_c.clamp(min=1e-30)).max()
    print("%s: sample mean off by at most %.2f standard errors, sample covariance by %.2f" % (what, float(zm), float(zc)))
    assert bool(((sm - mean).abs() <= 6 * se_m).all()), what + ": sample mean"
    assert bool(((sc - cov).abs() <= 6 * se_c).all()), what + ": sample covariance"


@pytest.mark.parametrize("C,diag", [(3, 0), (3, 1), (1, 0)])
def test_gaussian_samples_have_the_posteriors_moments(C, diag):
    S = 4096
    no, y, npar, est = op_inputs("gauss25", "known", C, diag, B=1, H=4, W=6)
    m = posterior_ref(no, y, npar, "gauss25", "known", est, diag)
    r = posterior_op(no, y, npar, "gauss25", "known", est, diag=diag, n_samples=S, seed=20261018, offset=1, want=("samples",))
    x = r["samples"].cpu().double()[:, 0].permute(0, 2, 3, 1).reshape(S, 24, C)
    assert torch.isfinite(x).all()
    _moment_bounds(x, m["mean"][0].permute(1, 2, 0).reshape(24, C), full_matrix(m["cov"])[0].reshape(24, C, C), S, "gauss25 C %d diag %d" % (C, diag))


@pytest.mark.parametrize("C", [3, 1])
def test_impulse_samples_follow_the_mixture(C):
    """alpha 0.5, priors of |det U|^(1/C) ~ 0.4 (C = 3) / 0.3 (C = 1) and y within about one prior std dev of mu_x: the two components
    are about equally likely a posteriori"""
    S, H, W = 4096, 4, 6
    NA = C * (C + 1) // 2
    mu = R.hash_tensor((1, C, H, W), 901, 0.3, 0.7)
    A = R.hash_tensor((1, NA, H, W), 902, -0.1, 0.1)
    dgi = (0, 3, 5) if C == 3 else (0,)
    A[:, dgi] = R.hash_tensor((1, C, H, W), 903, 0.3, 0.5) if C == 3 else R.hash_tensor((1, 1, H, W), 903, 0.2, 0.4)
    t = R.hash_tensor((1, C, H, W), 904, -1.0, 1.0)
    if C == 3:
        y = torch.stack([mu[:, 0] + A[:, 0] * t[:, 0] + A[:, 1] * t[:, 1] + A[:, 2] * t[:, 2], mu[:, 1] + A[:, 3] * t[:, 1] + A[:, 4] * t[:, 2],
                         mu[:, 2] + A[:, 5] * t[:, 2]], 1)
    else:
        y = mu + A * t
    no, npar = torch.cat([mu, A], 1), torch.full((1,), 0.5)
    m = posterior_ref(no, y, npar, "impulse", "known", None)
    w = m["w"].reshape(-1)
    mid = (w > 0.1) & (w < 0.9)
    print("mirror: w in (0.1, 0.9) at %d of %d pixels (w from %.3f to %.3f)" % (int(mid.sum()), w.numel(), float(w.min()), float(w.max())))
    assert int(mid.sum()) * 2 >= w.numel()
    r = posterior_op(no, y, npar, "impulse", "known", None, n_samples=S, seed=77, offset=3, want=("samples",))
    x = r["samples"].cpu()[:, 0].permute(0, 2, 3, 1).reshape(S, H * W, C)
    assert torch.isfinite(x).all()
    yy = y[0].permute(1, 2, 0).reshape(H * W, C)
    is_y = (x == yy[None]).all(-1)                                    # exactly the noisy pixel, in every channel
    share = is_y.double().mean(0)
    se = (w * (1 - w) / S).sqrt()
    print("share of samples equal to y: off by at most %.2f binomial standard errors" % float(((share - w).abs() / se).max()))
    assert bool(((share - w).abs() <= 6 * se).all())
    pm = m["prior_mean"][0].permute(1, 2, 0).reshape(H * W, C)
    pc = full_matrix(m["prior_cov"])[0].reshape(H * W, C, C)
    n_other = (~is_y).sum(0)
    assert int((n_other >= 200).sum()) * 2 >= H * W
    for p in range(H * W):
        if int(n_other[p]) >= 200:
            xs = x[~is_y[:, p], p].double()[:, None, :]
            _moment_bounds(xs, pm[p:p + 1], pc[p:p + 1], xs.shape[0], "impulse C %d pixel %d (%d prior samples)" % (C, p, xs.shape[0]))


# ---- Denoiser.posterior ------------------------------------------------------------------------------------------------------------------
def _denoiser(style, mode, ch):
    """blind-spot Denoiser, main network from R.make_params(seed 5), sigma network (var) from seed 6, learnt constant (const) at 1.7"""
    from ssdn.denoiser import Denoiser
    d = Denoiser(impulse_cfg(style, mode, ch), device="cuda:0")
    d.get_model(Denoiser.MODEL, False).load_state_dict(R.reference_state_dict(R.make_params(ch, ch + ch * (ch + 1) // 2, True, seed=5)))
    if mode == "var":
        d.get_model(Denoiser.SIGMA_ESTIMATOR, False).load_state_dict(R.reference_state_dict(R.make_params(ch, 1, False, seed=6)))
    if mode == "const":
        with torch.no_grad():
            d.l_params[Denoiser.ESTIMATED_SIGMA].fill_(1.7)
    d.mark_dirty()
    return d


def _batch(style, ch, B=2, Psz=32, seed=0):
    from ssdn.datasets import NoisyDataset
    MD = NoisyDataset.Metadata
    clean = R.hash_tensor((B, ch, Psz, Psz), 61 + seed, 0, 1)
    noisy = torch.clamp(clean + R.hash_tensor((B, ch, Psz, Psz), 62 + seed, -1, 1) * 0.17, 0, 1)
    npv = {"gauss25": 25 / 255.0, "poisson30": 30.0, "impulse50": 0.5}[style]
    return [noisy.to(DEV), clean.to(DEV), {MD.CLEAN: clean, MD.INPUT_NOISE_VALUES: torch.full((B, 1, 1, 1), npv)}]


DEN_CASES = [("gauss25", "known", 3), ("impulse50", "const", 3), ("poisson30", "var", 1)]


@pytest.mark.parametrize("style,mode,ch", DEN_CASES)
def test_denoiser_posterior_outputs_and_side_effects(style, mode, ch):
    from ssdn.params import PipelineOutput as PO
    d = _denoiser(style, mode, ch)
    data = _batch(style, ch)
    B, S = 2, 32
    d.eval()
    keys = (PO.IMG_DENOISED, PO.IMG_MU, PO.MODEL_STD_DEV, PO.NOISE_STD_DEV)
    with torch.no_grad():
        before = d.run_pipeline(data)
    eng = d._engines[(B, S, S, False, 64)][0]
    blob = eng.export_plan()
    d.train()                                   # whatever the module's mode
    post = d.posterior(data, samples=3, seed=5, offset=2)
    assert d.training and d._last_train_engine is None and not eng._post["cov"].requires_grad
    assert set(post) == {"mean", "cov", "std", "samples"} and not any(v.requires_grad for v in post.values())
    assert post["cov"].shape == (B, ch * (ch + 1) // 2, S, S) and post["std"].shape == (B, ch, S, S) and post["samples"].shape == (3, B, ch, S, S)
    assert torch.equal(post["mean"], before[PO.IMG_DENOISED])
    if mode != "known":                                                      # (mode known reads the noise level from the metadata)
        assert set(d.posterior(data[0])) == {"mean", "cov", "std"}           # a bare BCHW batch, no samples
    assert eng.export_plan() == blob
    # fresh tensors: another call does not change what the first returned
    kept = {k: v.clone() for k, v in post.items()}
    again = d.posterior(data, samples=3, seed=5, offset=2)
    assert all(torch.equal(post[k], kept[k]) and torch.equal(again[k], kept[k]) and again[k].data_ptr() != post[k].data_ptr() for k in kept)
    assert not torch.equal(d.posterior(data, samples=3, seed=5, offset=3)["samples"], kept["samples"])
    # teacher-forced: the mirror on the engine's own network output and noise estimate
    no, y, npar = eng.main.tensor("out32").cpu(), eng.inp.cpu(), eng.noise_param.cpu()
    est = eng.est_raw.cpu() if mode == "var" else d.l_params[d.ESTIMATED_SIGMA].detach().cpu().reshape(1) if mode == "const" else None
    st = "impulse" if is_impulse(style) else style
    m = posterior_ref(no, y, npar, st, mode, est)
    fig = fp32_yardstick(no, y, npar, st, mode, est, 0, m)
    close(post["cov"], m["cov"], 2e-5, _atol(1e-6 * float(m["cov"].abs().max()), fig["cov"]), "cov, teacher-forced")
    close(post["std"], m["std"], 2e-5, _atol(1e-6 * float(m["std"].abs().max()), fig["std"]), "std, teacher-forced")
    d.eval()
    with torch.no_grad():
        after = d.run_pipeline(data)
    for k in keys:
        assert torch.equal(after[k], before[k]), k


def test_posterior_between_train_steps_leaves_the_weights_alone():
    data = [_batch("gauss25", 3, seed=k) for k in range(3)]

    def run(with_posterior):
        d = _denoiser("gauss25", "known", 3)
        d.train()
        for k in range(3):
            d.train_step(data[k], lr=3e-4)
            if with_posterior and k < 2:
                d.posterior(data[k], samples=2, seed=k)
        torch.cuda.synchronize()
        return d.flat.detach().clone(), d.adam_m.clone()
    w0, m0 = run(False)
    w1, m1 = run(True)
    assert torch.isfinite(w0).all() and torch.equal(w0, w1) and torch.equal(m0, m1)


def test_cli_eval_posterior_writes_std_maps_and_samples(tmp_path):
    """one `ssdn eval --posterior 2` over a folder of two images, one of them non-square (loader workers off: their start-up is most of an
    evaluation this small)"""
    from PIL import Image
    from ssdn.__main__ import start_cli
    from ssdn.params import ConfigValue
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    sizes = [(40, 24), (32, 32)]                                        # (w, h)
    for i, (w, h) in enumerate(sizes):
        a = (R.hash_tensor((h, w, 3), 700 + i, 0, 1).numpy() * 255).astype(np.uint8)
        Image.fromarray(a, mode="RGB").save(imgs / ("im%d.png" % i))
    d = _denoiser("gauss25", "known", 3)
    d.cfg[ConfigValue.DATALOADER_WORKERS] = 0
    torch.save({k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in d.state_dict().items()}, tmp_path / "model.wt")
    ev = start_cli(["eval", "-m", str(tmp_path / "model.wt"), "-d", str(imgs), "--runs_dir", str(tmp_path / "runs"), "--batch_size", "2",
                    "--posterior", "2"])
    pdir = os.path.join(ev.run_dir_path, "posterior")
    assert sorted(os.listdir(pdir)) == sorted("img_%05d_%s" % (i, s) for i in range(2) for s in ("std.npy", "sample0.png", "sample1.png"))
    for i, (w, h) in enumerate(sizes):
        std = np.load(os.path.join(pdir, "img_%05d_std.npy" % i))
        assert std.dtype == np.float32 and std.shape == (3, h, w) and np.isfinite(std).all() and (std >= 0).all() and std.max() > 0
        for k in range(2):
            assert Image.open(os.path.join(pdir, "img_%05d_sample%d.png" % (i, k))).size == (w, h)
        assert Image.open(os.path.join(ev.run_dir_path, "eval_imgs", "img_%05d_out.png" % i)).size == (w, h)
    assert not np.array_equal(np.asarray(Image.open(os.path.join(pdir, "img_00000_sample0.png"))),
                              np.asarray(Image.open(os.path.join(pdir, "img_00000_sample1.png"))))
    with open(os.path.join(ev.run_dir_path, "psnrs.csv")) as fh:
        assert fh.readline() == "id,psnr_nsy,psnr_out,psnr_mu_out\n"              # the header of an evaluation without the flag
        rows = list(csv.DictReader(fh, fieldnames=["id", "psnr_nsy", "psnr_out", "psnr_mu_out"]))
    assert len(rows) == 2 and all(math.isfinite(float(r["psnr_out"])) for r in rows)
