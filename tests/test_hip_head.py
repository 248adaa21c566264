"""GPU parity of the loss heads and the optimiser kernels against the golden vectors generated from the reference
(tests/golden/g_head_*, g_mse, g_maskmse) and the oracle's Adam restatement.  fp32 kernels => tight tolerances."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import restate as R
from head_ops import P, head_op, head_vjp_op, run_one
from test_diag_cov_cpu import diag_inputs
from test_head_vjp_cpu import head_inputs, upstream
from test_impulse_cpu import impulse_inputs

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


@pytest.mark.parametrize("style,npar", [("gauss25", 25 / 255.0), ("poisson30", 30.0)])
@pytest.mark.parametrize("mode", ["known", "const", "var"])
@pytest.mark.parametrize("ch", [1, 3])
def test_ssdn_head_vs_reference(golden_dir, style, npar, mode, ch):
    """Closed-form fp32 posterior head.
    Primary: vs the oracle (restate.ssdn_head -- pinned to the reference on these very inputs by tests/test_oracle_golden)
    evaluated in FLOAT64: 2e-5.  Secondary: vs the reference's own fp32 outputs (golden): loss/gradients 5e-4; the posterior
    mean only to 5e-3 abs, because the reference's fp32 LU inverse of the near-singular Sigma_x + 1e-6 I is itself off by
    up to 4.6e-4 from the exact value on these inputs (measured), while the kernel's algebraically equal
    mu + Sx (Sx+Sn)^-1 (y-mu) form stays within 2e-6 of it."""
    from ssdn.hip import lib as L
    g = np.load(os.path.join(golden_dir, "g_head_%s_%s_c%d.npz" % (style, mode, ch)))
    B, H = 2, 8
    ncomp = ch + ch * (ch + 1) // 2
    net_out = R.hash_tensor((B, ncomp, H, H), 41 + ch, -0.4, 0.6)
    net_out[:, :ch] = R.hash_tensor((B, ch, H, H), 42, 0.05, 0.95)
    noisy = R.hash_tensor((B, ch, H, H), 43, 0.0, 1.0)
    f = dict(dtype=torch.float32, device=dev())
    d_np = torch.full((B,), npar, **f)
    est_raw = None
    if mode == "var":
        raw_map = R.hash_tensor((B, 1, H, H), 44, 1.0, 3.0).to(dev())
        est_raw = torch.zeros(B, **f)
        run_one("spatial_mean", L.SpatialMeanArgs(P(raw_map), P(est_raw), B, H * H))
        np.testing.assert_allclose(est_raw.cpu().numpy(), raw_map.mean(dim=(1, 2, 3)).cpu().numpy(), rtol=1e-6)
    if mode == "const":
        est_raw = torch.full((1,), 1.7, **f)
    r = head_op(net_out, noisy, d_np, style, mode, est_raw)
    loss, mu, pme, mstd, nstd = r["loss"], r["mu"], r["pme"], r["model_std"], r["noise_std"]
    gno, g_est, g_sig, gmax = r["g_net_out"], r["g_est"], r["g_sig"], r["gmax"]

    def close(a, b, rtol, atol):
        b = b.detach().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
        np.testing.assert_allclose(a.cpu().numpy().reshape(b.shape), b, rtol=rtol, atol=atol)

    # ---- primary: float64 oracle ----
    no64 = net_out.double().requires_grad_(True)
    raw64 = est64 = None
    if mode == "var":
        raw64 = R.hash_tensor((B, 1, H, H), 44, 1.0, 3.0).double().requires_grad_(True)
        est64 = raw64.mean(dim=(2, 3), keepdim=True)
    if mode == "const":
        raw64 = torch.full((1, 1, 1, 1), 1.7, dtype=torch.float64, requires_grad=True)
        est64 = raw64
    o = R.ssdn_head(no64, noisy.double(), torch.full((B, 1, 1, 1), npar, dtype=torch.float64), style, mode, est64)
    o["loss"].mean().backward()
    close(loss, o["loss"], 2e-5, 1e-6)
    close(pme, o["out"], 2e-5, 5e-6)
    close(mstd, o["model_std"], 2e-5, 1e-6)
    close(gno, no64.grad, 2e-4, 1e-6 * float(no64.grad.abs().max()))
    if mode == "const":
        close(g_est[:1], raw64.grad.reshape(1), 2e-4, 1e-9)
    if mode == "var":
        close(g_sig, raw64.grad, 2e-4, 1e-10)

    # ---- secondary: the reference's own fp32 numbers ----
    close(loss, g["loss"], 2e-4, 1e-5)
    close(mu, g["out_mu"], 0, 0)
    close(pme, g["out"], 0, 5e-3)
    close(mstd, g["model_std"], 1e-3, 1e-4)
    if style.startswith("poisson"):
        close(nstd, g["noise_std"], 2e-4, 1e-6)
    else:
        want = g["noise_std"].reshape(-1)
        got = nstd.cpu().numpy()
        np.testing.assert_allclose(got[: len(want)] if len(want) == B else got[:1], want, rtol=2e-4)
    scale = float(np.abs(g["g_net_out"]).max())
    close(gno, g["g_net_out"], 5e-4, 1e-5 * scale)
    assert float(np.float32(np.abs(g["g_net_out"]).max())) == pytest.approx(float(np.int32(gmax[0].item()).view(np.float32)), rel=1e-3)
    if mode == "const":
        close(g_est[:1], g["g_raw"].reshape(1), 5e-4, 1e-8)
    if mode == "var":
        close(g_sig, g["g_raw"], 5e-4, 1e-9)


# head kind, channels, style, mode
CHUNK_CASES = [("full", 1, "gauss25", "known"), ("full", 1, "poisson30", "const"), ("full", 3, "gauss25", "known"),
               ("full", 3, "poisson30", "const"), ("diag", 3, "gauss25", "var"), ("impulse", 1, "impulse", "known"),
               ("impulse", 3, "impulse", "known")]


@pytest.mark.parametrize("kind,ch,style,mode", CHUNK_CASES)
def test_head_chunking_does_not_change_a_pixel(kind, ch, style, mode):
    """529 pixels per sample in 1, 2 and 3 blocks of 256 threads: a block's pixel loop makes up to three trips and its last trip, and the
    last block (265 / 264 and 177 / 177 / 175 pixels), are ragged.  What a kernel writes per pixel is the same bits however the pixels are
    dealt out; loss, g_est and g_sigma_out are the same sums in another order (rtol 1e-5, as for the re-association in
    tests/test_hip_diag_cov.py::test_diag_head_vjp_op_vs_float64)."""
    B, H = 3, 23
    if kind == "diag":
        net_out, noisy, npar, raw = diag_inputs(style, mode, B=B, H=H)
    elif kind == "impulse":
        net_out, noisy, npar, raw = impulse_inputs(ch, mode, 0.5, B=B, H=H)
    else:
        net_out, noisy, npar, raw = head_inputs(ch, style, mode, B=B, H=H)
    est_raw = raw.mean(dim=(1, 2, 3)) if mode == "var" else raw
    w, gp, gm = upstream(B, ch, H, seed=29 + ch)
    diag = int(kind == "diag")
    fwd, vjp = {}, {}
    for n in (1, 2, 3):
        fwd[n] = head_op(net_out, noisy, npar, style, mode, est_raw, diag=diag, nchunks=n)
        vjp[n] = head_vjp_op(net_out, noisy, npar, style, mode, est_raw, w, gp, gm, diag=diag, nchunks=n)
    pixel_f, pixel_v = ("mu", "pme", "model_std", "noise_std", "g_net_out"), ("g_net_out", "g_noisy")
    for k in pixel_f:
        assert torch.isfinite(fwd[1][k]).all(), k
    for k in pixel_v:
        assert torch.isfinite(vjp[1][k]).all(), k
    sums = [("loss", fwd)] + ([("g_est", fwd), ("g_est", vjp)] if mode != "known" else []) + ([("g_sig", fwd), ("g_sig", vjp)] if mode == "var" else [])
    for n in (2, 3):
        for k in pixel_f:
            assert torch.equal(fwd[n][k], fwd[1][k]), "forward %s, nchunks %d: %d elements differ" % (k, n, int((fwd[n][k] != fwd[1][k]).sum()))
        for k in pixel_v:
            assert torch.equal(vjp[n][k], vjp[1][k]), "vjp %s, nchunks %d: %d elements differ" % (k, n, int((vjp[n][k] != vjp[1][k]).sum()))
        for k, runs in sums:
            a, b = runs[n][k].cpu().double().numpy(), runs[1][k].cpu().double().numpy()
            print("%s %s nchunks %d vs 1: max rel diff %.3e" % ("forward" if runs is fwd else "vjp", k, n, float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))))
            np.testing.assert_allclose(a, b, rtol=1e-5, atol=0)


def test_mse_and_masked_mse_vs_reference(golden_dir):
    from ssdn.hip import lib as L
    f = dict(dtype=torch.float32, device=dev())
    out = R.hash_tensor((3, 3, 16, 16), 51, 0, 1).to(dev())
    tgt = R.hash_tensor((3, 3, 16, 16), 52, 0, 1).to(dev())
    g = np.load(os.path.join(golden_dir, "g_mse.npz"))
    loss, grad = torch.zeros(3, **f), torch.zeros(3, 3, 16, 16, **f)
    gmax = torch.zeros(4, dtype=torch.int32, device=dev())
    run_one("mse", L.MseArgs(P(out), P(tgt), None, 0, 3, 3, 16, 16, P(loss), P(grad), P(gmax)))
    np.testing.assert_allclose(loss.cpu().numpy().reshape(3, 1), g["loss"], rtol=1e-5)
    np.testing.assert_allclose(grad.cpu().numpy(), g["g_out"], rtol=1e-5, atol=1e-9)
    g = np.load(os.path.join(golden_dir, "g_maskmse.npz"))
    coords = torch.from_numpy(g["coords"])[0].contiguous().to(dev())      # batch element 0's coordinates (reference quirk)
    loss, grad = torch.zeros(3, **f), torch.full((3, 3, 16, 16), float("nan"), **f)
    run_one("mask_mse", L.MseArgs(P(out), P(tgt), P(coords), 64, 3, 3, 16, 16, P(loss), P(grad), P(gmax)))
    np.testing.assert_allclose(loss.cpu().numpy().reshape(3, 1), g["loss"], rtol=1e-5)
    np.testing.assert_allclose(grad.cpu().numpy(), g["g_out"], rtol=1e-5, atol=1e-9)


# coordinates (row, col) as include/ssdn_hip.h documents them for ssdn_mse_args.coords: several rows (16x24: columns) are >= 16, so a lookup
# that swaps the two lands on another pixel or off the plane (which the kernel skips); (20, 13) / (13, 20) twice: duplicates count twice
@pytest.mark.parametrize("H,W,coords", [(16, 24, [(0, 0), (15, 23), (3, 17), (9, 20), (12, 16), (2, 5), (13, 20), (13, 20), (7, 23), (15, 1)]),
                                        (24, 16, [(0, 0), (23, 15), (17, 3), (20, 9), (16, 12), (5, 2), (20, 13), (20, 13), (23, 7), (1, 15)])])
def test_mse_and_masked_mse_on_a_non_square_plane(H, W, coords):
    """SSDN_OP_MSE / SSDN_OP_MASK_MSE with H != W against float64 torch (oracle/restate.py's formulas: mean over C, H, W; masked: squared
    errors summed over the coordinates, mean over C), gradient of mean_b(loss) compared in full from a NaN start"""
    from ssdn.hip import lib as L
    f = dict(dtype=torch.float32, device=dev())
    B, Cn = 3, 3
    out, tgt = R.hash_tensor((B, Cn, H, W), 51, 0, 1), R.hash_tensor((B, Cn, H, W), 52, 0, 1)
    o64 = out.double().requires_grad_(True)
    want = ((o64 - tgt.double()) ** 2).reshape(B, -1).mean(1)
    want.mean().backward()
    loss, grad = torch.zeros(B, **f), torch.full((B, Cn, H, W), float("nan"), **f)
    gmax = torch.zeros(4, dtype=torch.int32, device=dev())
    dout, dtgt = out.to(dev()), tgt.to(dev())
    run_one("mse", L.MseArgs(P(dout), P(dtgt), None, 0, B, Cn, H, W, P(loss), P(grad), P(gmax)))
    np.testing.assert_allclose(loss.cpu().numpy(), want.detach().numpy(), rtol=1e-5)
    np.testing.assert_allclose(grad.cpu().numpy(), o64.grad.numpy(), rtol=1e-5, atol=1e-9)
    assert float(np.int32(gmax[0].item()).view(np.float32)) == pytest.approx(float(o64.grad.abs().max()), rel=1e-5)
    c = torch.tensor(coords, dtype=torch.int64)
    o64 = out.double().requires_grad_(True)
    diff = tgt.double()[:, :, c[:, 0], c[:, 1]] - o64[:, :, c[:, 0], c[:, 1]]
    want = (diff ** 2).sum(-1).mean(1)
    want.mean().backward()
    dc = c.contiguous().to(dev())
    loss, grad = torch.zeros(B, **f), torch.full((B, Cn, H, W), float("nan"), **f)
    run_one("mask_mse", L.MseArgs(P(dout), P(dtgt), P(dc), len(coords), B, Cn, H, W, P(loss), P(grad), P(gmax)))
    np.testing.assert_allclose(loss.cpu().numpy(), want.detach().numpy(), rtol=1e-5)
    np.testing.assert_allclose(grad.cpu().numpy(), o64.grad.numpy(), rtol=1e-5, atol=1e-9)
    assert int((grad != 0).sum()) == B * Cn * (len(set(coords)))


def test_fused_adam_vs_oracle():
    from ssdn.hip import lib as L
    n = 100003
    p0 = R.hash_tensor((n,), 1, -1, 1)
    p, m, v = p0.clone(), torch.zeros(n), torch.zeros(n)
    dp, dm, dv = p0.to(dev()), torch.zeros(n, device=dev()), torch.zeros(n, device=dev())
    for step in range(1, 4):
        g = R.hash_tensor((n,), 10 + step, -1, 1) * 10.0 ** (-step)
        lr = 3e-4 * step
        R.adam_step(p, g, m, v, step, lr)
        dg = g.to(dev())
        run_one("adam", L.AdamArgs(P(dp), P(dg), P(dm), P(dv), n, lr, 0.9, 0.99, 1e-8, 1 - 0.9 ** step, 1 - 0.99 ** step, 1.0))
    np.testing.assert_allclose(dp.cpu().numpy(), p.numpy(), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(dv.cpu().numpy(), v.numpy(), rtol=1e-5, atol=1e-12)


def test_metrics_kernel_vs_reference_psnr_and_host_formulas(golden_dir):
    """SSDN_OP_METRICS (H11): per-sample PSNR against the reference-generated golden values, and the accumulated sums / counts of two
    launches against the host formulas the reference trainer applies every step (train.py:205-218 with Metric.add)."""
    from ssdn.hip import lib as L
    a = R.hash_tensor((3, 3, 16, 16), 71, 0, 1)
    b = torch.clamp(a + R.hash_tensor((3, 3, 16, 16), 72, -0.1, 0.1), 0, 1)
    mu = torch.clamp(a + R.hash_tensor((3, 3, 16, 16), 73, -0.2, 0.2), 0, 1)
    loss = R.hash_tensor((3,), 74, -1, 1)
    mstd = R.hash_tensor((3, 16, 16), 75, 0, 0.1)
    nstd = R.hash_tensor((3,), 76, 0.05, 0.2)
    d = lambda t: t.to(dev()).contiguous()   # noqa: E731
    da, db, dmu, dl, dm, dn = d(a), d(b), d(mu), d(loss), d(mstd), d(nstd)
    per = torch.zeros(3, 8, device=dev())
    acc = torch.zeros(16, device=dev())
    args = L.MetricsArgs(P(db), P(dmu), P(da), P(dl), P(dm), P(dn), None, 3, 3, 16, 16, 3, P(per), P(acc))
    run_one("metrics", args)
    np.testing.assert_allclose(per[:, 1].cpu().numpy(), np.load(os.path.join(golden_dir, "g_psnr.npz"))["psnr"], rtol=1e-5)
    run_one("metrics", args)                       # accumulates
    psnr = lambda x: (-10 * torch.log10(((x - a) ** 2).reshape(3, -1).mean(1)))   # noqa: E731
    want = [2 * float(loss.sum()), 2 * float(psnr(b).sum()), 2 * float(psnr(mu).sum()), 2 * float((nstd * 255).sum()),
            2 * float((mstd * 255).reshape(3, -1).mean(1).sum())]
    got = acc.cpu().numpy()
    np.testing.assert_allclose(got[0:10:2], want, rtol=2e-5)
    assert list(got[1:10:2]) == [6.0] * 5 and got[15] == 0
    # padded evaluation batch: PSNR over each sample's valid extent only; one noise level for the whole batch counts once
    ext = torch.tensor([[16, 16], [10, 12], [5, 16]], dtype=torch.int32, device=dev())
    acc.zero_()
    args2 = L.MetricsArgs(P(db), None, P(da), None, None, P(dn), P(ext), 3, 3, 16, 16, 1, P(per), P(acc))
    run_one("metrics", args2)
    want_p = [float(-10 * torch.log10(((b[i, :, :e1, :e2] - a[i, :, :e1, :e2]) ** 2).mean())) for i, (e1, e2) in enumerate([(16, 16), (10, 12), (5, 16)])]
    np.testing.assert_allclose(per[:, 1].cpu().numpy(), want_p, rtol=2e-5)
    got = acc.cpu().numpy()
    assert got[1] == 0 and got[3] == 3 and got[5] == 0 and got[7] == 1 and got[9] == 0
    np.testing.assert_allclose(got[6], float(nstd[0]) * 255, rtol=1e-6)


@pytest.mark.parametrize("H,W,exts", [(16, 24, [(16, 24), (10, 20), (5, 24)]), (24, 16, [(24, 16), (20, 10), (24, 5)])])
def test_metrics_kernel_on_a_non_square_plane(H, W, exts):
    """SSDN_OP_METRICS with H != W: the whole plane and per-sample valid extents (e1 rows, e2 columns; one of them reaches past the
    plane's other side, so swapped extents or a swapped row pitch crop other pixels) against the host PSNR formula in float64"""
    from ssdn.hip import lib as L
    a = R.hash_tensor((3, 3, H, W), 71, 0, 1)
    b = torch.clamp(a + R.hash_tensor((3, 3, H, W), 72, -0.1, 0.1), 0, 1)
    mu = torch.clamp(a + R.hash_tensor((3, 3, H, W), 73, -0.2, 0.2), 0, 1)
    loss = R.hash_tensor((3,), 74, -1, 1)
    mstd = R.hash_tensor((3, H, W), 75, 0, 0.1)
    nstd = R.hash_tensor((3,), 76, 0.05, 0.2)
    d = lambda t: t.to(dev()).contiguous()   # noqa: E731
    da, db, dmu, dl, dm, dn = d(a), d(b), d(mu), d(loss), d(mstd), d(nstd)
    per = torch.zeros(3, 8, device=dev())
    acc = torch.zeros(16, device=dev())
    args = L.MetricsArgs(P(db), P(dmu), P(da), P(dl), P(dm), P(dn), None, 3, 3, H, W, 3, P(per), P(acc))
    run_one("metrics", args)
    run_one("metrics", args)                       # accumulates
    psnr = lambda x: (-10 * torch.log10(((x.double() - a.double()) ** 2).reshape(3, -1).mean(1)))   # noqa: E731
    np.testing.assert_allclose(per[:, 1].cpu().numpy(), psnr(b).numpy(), rtol=2e-5)
    want = [2 * float(loss.sum()), 2 * float(psnr(b).sum()), 2 * float(psnr(mu).sum()), 2 * float((nstd * 255).sum()),
            2 * float((mstd * 255).reshape(3, -1).mean(1).sum())]
    got = acc.cpu().numpy()
    np.testing.assert_allclose(got[0:10:2], want, rtol=2e-5)
    assert list(got[1:10:2]) == [6.0] * 5 and got[15] == 0
    ext = torch.tensor(exts, dtype=torch.int32, device=dev())
    acc.zero_()
    args2 = L.MetricsArgs(P(db), None, P(da), None, None, P(dn), P(ext), 3, 3, H, W, 1, P(per), P(acc))
    run_one("metrics", args2)
    want_p = [float(-10 * torch.log10(((b[i, :, :e1, :e2].double() - a[i, :, :e1, :e2].double()) ** 2).mean())) for i, (e1, e2) in enumerate(exts)]
    np.testing.assert_allclose(per[:, 1].cpu().numpy(), want_p, rtol=2e-5)
    got = acc.cpu().numpy()
    assert got[1] == 0 and got[3] == 3 and got[5] == 0 and got[7] == 1 and got[9] == 0
    np.testing.assert_allclose(got[2], sum(want_p), rtol=2e-5)
    np.testing.assert_allclose(got[6], float(nstd[0]) * 255, rtol=1e-6)
