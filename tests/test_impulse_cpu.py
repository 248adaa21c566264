"""CPU: the impulse noise model.  `impulse_head` restates the formulas of csrc/head_impulse.hip in torch -- the
sum-of-PSD form of Sigma_y, adjugate inverses, the posterior weight in the log domain, and the hand-derived vector-Jacobian product
-- in any dtype; in float64 it agrees with autograd of the PAPER's form of Sigma_y and the raw mixture posterior (`impulse_oracle`).
Then: the posterior mean beats both the noisy pixel and the prior mean on synthetic draws, the loss gradient has zero mean there, the
host data layer (style grammar, `add_impulse`, NoisyDataset, the CPU path of DevicePatchStream) and the plumbing that needs no GPU.
The GPU tests (tests/test_hip_impulse.py) reuse `impulse_inputs`, `impulse_head`, `impulse_oracle` and `impulse_cfg`."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import restate as R
import ssdn
from ssdn.denoiser import Denoiser
from ssdn.params import ConfigValue, NoiseAlgorithm, NoiseValue
from ssdn.utils import noise

MODES = ("known", "const", "var")
ALPHAS = (0.05, 0.5)
TERMS = ("all", "loss", "pme", "mu")


def impulse_cfg(style="impulse50", mode="known", ch=3, diag=False):
    cfg = ssdn.cfg.base()
    cfg[ConfigValue.ALGORITHM] = NoiseAlgorithm.SELFSUPERVISED_DENOISING
    cfg[ConfigValue.NOISE_STYLE] = style
    cfg[ConfigValue.NOISE_VALUE] = NoiseValue(mode)
    cfg[ConfigValue.IMAGE_CHANNELS] = ch
    cfg[ConfigValue.DIAGONAL_COVARIANCE] = diag
    return ssdn.cfg.infer(cfg, model_only=True)


def raw_of_alpha(alpha):
    """the pre-softplus estimate whose remap softplus(raw - 4) + 1e-3 is alpha"""
    return 4.0 + math.log(math.expm1(alpha - 1e-3))


def impulse_inputs(C, mode, alpha, B=2, H=8, seed=0):
    """net_out [B,C+C(C+1)/2,H,W] (means in (0.05, 0.95), A components in (-0.4, 0.6), a few pixels with zeroed components -- one with all
    of A zero), noisy, alpha [B], raw estimate (var: a map [B,1,H,W] around the value that gives alpha; const: [1]), all float32"""
    Cout = C + C * (C + 1) // 2
    net_out = R.hash_tensor((B, Cout, H, H), 241 + seed, -0.4, 0.6)
    net_out[:, :C] = R.hash_tensor((B, C, H, H), 242 + seed, 0.05, 0.95)
    net_out[0, C, 0, 0] = 0.0
    net_out[0, C:, 1, 2] = 0.0                      # Sigma_x = 0
    if C == 3:
        net_out[1, 7:9, 2, 3] = 0.0
        net_out[1, 8, 4, 4] = -0.35
        net_out[0, 5, 3, 5] = 0.0
    noisy = R.hash_tensor((B, C, H, H), 243 + seed, 0.0, 1.0)
    noisy[1, :, 5, 5] = net_out[1, :C, 5, 5] + 0.01                 # a pixel close to its prior mean: w near 1
    npar = torch.full((B,), float(alpha))
    raw = None
    if mode == "var":
        raw = R.hash_tensor((B, 1, H, H), 244 + seed, -0.5, 0.5) + raw_of_alpha(alpha)
    elif mode == "const":
        raw = torch.full((1,), raw_of_alpha(alpha))
    return net_out, noisy, npar, raw


# ---- the kernels' formulas ----------------------------------------------------------------------------------------------------------------
def _alpha(npar, mode, est_raw, B, dtype):
    """alpha [B] as the head sees it, d alpha / d est_raw [B]"""
    if mode == "known":
        return npar.to(dtype).reshape(B).clamp(1e-3, 0.999), None
    raw = est_raw.to(dtype).reshape(-1)
    raw = raw.expand(B) if raw.numel() == 1 else raw
    sp = F.softplus(raw - 4.0) + 1e-3
    return sp.clamp(max=0.999), torch.where(sp < 0.999, torch.sigmoid(raw - 4.0), torch.zeros_like(sp))


def _sym_adj(s):
    s00, s01, s02, s11, s12, s22 = s
    c = (s11 * s22 - s12 * s12, s02 * s12 - s01 * s22, s01 * s12 - s02 * s11, s00 * s22 - s02 * s02, s01 * s02 - s00 * s12,
         s00 * s11 - s01 * s01)
    return c, s00 * c[0] + s01 * c[1] + s02 * c[2]


def _sym_mv(m, v, k=1.0):
    m00, m01, m02, m11, m12, m22 = m
    return [(m00 * v[0] + m01 * v[1] + m02 * v[2]) * k, (m01 * v[0] + m11 * v[1] + m12 * v[2]) * k, (m02 * v[0] + m12 * v[1] + m22 * v[2]) * k]


def impulse_head(net_out, noisy, npar, mode, est_raw, w=None, g_pme=None, g_mu=None, dtype=torch.float64):
    """k_head_impulse / k_head_vjp_impulse per pixel, in `dtype`.  est_raw: [1] (const) or [B] (var) pre-softplus.
    -> dict: loss [B], mu, pme [B,C,H,W], model_std [B,H,W], alpha [B], and for the upstream gradients w = dL/dLOSS [B], g_pme, g_mu:
    g_net_out = dL/dnet_out, g_est = dL/dest_raw ([1] const, [B] var, None known), g_noisy = the head's direct dL/dnoisy"""
    cv = lambda t: None if t is None else t.to(dtype)    # noqa: E731
    no, y, w, gp, gm = cv(net_out), cv(noisy), cv(w), cv(g_pme), cv(g_mu)
    B, Cout, H, W = no.shape
    C = 1 if Cout == 2 else 3
    HW = H * W
    alpha_b, dalpha_draw = _alpha(npar, mode, est_raw, B, dtype)
    al = alpha_b.view(B, 1, 1)
    om, k = 1 - al, al * (1 - al)
    lodds = torch.log(om) - torch.log(al)
    reg = 0.1 if mode != "known" else 0.0
    sc = (w if w is not None else torch.zeros(B, dtype=dtype)).view(B, 1, 1) / HW
    mu = [no[:, c] for c in range(C)]
    A = [no[:, C + c] for c in range(Cout - C)]
    yy = [y[:, c] for c in range(C)]
    gpl = None if gp is None else [gp[:, c] for c in range(C)]
    e = [m - 0.5 for m in mu]
    d = [yy[c] - (0.5 * al + om * mu[c]) for c in range(C)]
    r = [yy[c] - mu[c] for c in range(C)]
    out = {}
    if C == 1:
        a, sx = A[0], A[0] * A[0]
        sy = om * sx + al / 12 + k * e[0] * e[0]
        q = d[0] / sy
        l = torch.log(sy) + d[0] * q - reg * al
        G = sc * (1 / sy - q * q)
        gmu = [-2 * sc * om * q + 2 * k * G * e[0]]
        gx = om * G
        galpha = 2 * sc * q * e[0] + G * (1 / 12 - sx + (1 - 2 * al) * e[0] * e[0]) - reg * sc
        gy = [2 * sc * q]
        sp = sx + 1e-6
        t = r[0] / sp
        z = lodds - 0.5 * torch.log(sp) - 0.5 * r[0] * t - 0.5 * math.log(2 * math.pi)
        wt, wm = torch.sigmoid(z), torch.sigmoid(-z)
        pme = [mu[0] + wt * r[0]]
        if gpl is not None:
            s = gpl[0] * r[0] * wt * wm
            gmu[0] = gmu[0] + gpl[0] * wm + s * t
            gx = gx + 0.5 * s * (t * t - 1 / sp)
            galpha = galpha - s / k
            gy[0] = gy[0] + gpl[0] * wt - s * t
        gA = [2 * a * gx]
        mstd = a.abs()
    else:
        x = (A[0] * A[0] + A[1] * A[1] + A[2] * A[2], A[1] * A[3] + A[2] * A[4], A[2] * A[5], A[3] * A[3] + A[4] * A[4], A[4] * A[5], A[5] * A[5])
        dg = al / 12
        s_ = (om * x[0] + dg + k * e[0] * e[0], om * x[1] + k * e[0] * e[1], om * x[2] + k * e[0] * e[2],
              om * x[3] + dg + k * e[1] * e[1], om * x[4] + k * e[1] * e[2], om * x[5] + dg + k * e[2] * e[2])
        cf, det = _sym_adj(s_)
        rdet = 1 / det
        q = _sym_mv(cf, d, rdet)
        l = 0.5 * torch.log(det) + 0.5 * (d[0] * q[0] + d[1] * q[1] + d[2] * q[2]) - reg * al
        hs = 0.5 * sc
        ij = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
        G = tuple(hs * (cf[n] * rdet - q[i] * q[j]) for n, (i, j) in enumerate(ij))
        Ge = _sym_mv(G, e)
        gmu = [-sc * om * q[c] + 2 * k * Ge[c] for c in range(3)]
        gy = [sc * q[c] for c in range(3)]
        gx = [om * g for g in G]
        gdotx = G[0] * x[0] + G[3] * x[3] + G[5] * x[5] + 2 * (G[1] * x[1] + G[2] * x[2] + G[4] * x[4])
        galpha = (sc * (q[0] * e[0] + q[1] * e[1] + q[2] * e[2]) + (G[0] + G[3] + G[5]) / 12 - gdotx
                  + (1 - 2 * al) * (e[0] * Ge[0] + e[1] * Ge[1] + e[2] * Ge[2]) - reg * sc)
        sp = (x[0] + 1e-6, x[1], x[2], x[3] + 1e-6, x[4], x[5] + 1e-6)
        cp, detp = _sym_adj(sp)
        detp = detp.clamp(min=1e-18)
        rdp = 1 / detp
        t = _sym_mv(cp, r, rdp)
        quad = (r[0] * t[0] + r[1] * t[1] + r[2] * t[2]).clamp(min=0)
        z = lodds - 0.5 * torch.log(detp) - 0.5 * quad - 1.5 * math.log(2 * math.pi)
        wt, wm = torch.sigmoid(z), torch.sigmoid(-z)
        pme = [mu[c] + wt * r[c] for c in range(3)]
        if gpl is not None:
            s = (gpl[0] * r[0] + gpl[1] * r[1] + gpl[2] * r[2]) * wt * wm
            for c in range(3):
                gmu[c] = gmu[c] + gpl[c] * wm + s * t[c]
                gy[c] = gy[c] + gpl[c] * wt - s * t[c]
            gx = [gx[n] + 0.5 * s * (t[i] * t[j] - cp[n] * rdp) for n, (i, j) in enumerate(ij)]
            galpha = galpha - s / k
        gA = [2 * (gx[0] * A[0]), 2 * (gx[0] * A[1] + gx[1] * A[3]), 2 * (gx[0] * A[2] + gx[1] * A[4] + gx[2] * A[5]),
              2 * (gx[1] * A[1] + gx[3] * A[3]), 2 * (gx[1] * A[2] + gx[3] * A[4] + gx[4] * A[5]),
              2 * (gx[2] * A[2] + gx[4] * A[4] + gx[5] * A[5])]
        mstd = (A[0] * A[3] * A[5]).abs() ** (1 / 3)
    if gm is not None:
        gmu = [gmu[c] + gm[:, c] for c in range(C)]
    out.update(loss=l.reshape(B, -1).mean(1), mu=torch.stack(mu, 1), pme=torch.stack(pme, 1), model_std=mstd, alpha=alpha_b,
               g_net_out=torch.stack(gmu + gA, 1), g_noisy=torch.stack(gy, 1), g_est=None)
    if mode != "known":
        gest = galpha.reshape(B, -1).sum(1) * dalpha_draw
        out["g_est"] = gest.sum().view(1) if mode == "const" else gest
    return out


# ---- float64 autograd of the paper's form ---------------------------------------------------------------------------------------------------
def _sigma_x(A, C):
    B, _, H, W = A.shape
    if C == 1:
        return (A[:, 0] ** 2)[..., None, None]
    U = torch.zeros((B, H, W, 3, 3), dtype=A.dtype)
    for n, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        U[..., i, j] = A[:, n]
    return U @ U.transpose(-1, -2)


def impulse_forward_paper(no, y, alpha_b, reg):
    """loss [B], pme, mu from the PAPER's Sigma_y = alpha (I/12 + 1/4 11^T) + (1 - alpha)(Sigma_x + mu mu^T) - mu_y mu_y^T and the raw
    mixture posterior ((1 - alpha) f y + alpha mu) / ((1 - alpha) f + alpha), f = N(y; mu, Sigma_x + 1e-6 I); differentiable"""
    B, Cout, H, W = no.shape
    C = 1 if Cout == 2 else 3
    mu = no[:, :C].permute(0, 2, 3, 1)                          # [B,H,W,C]
    yv = y.permute(0, 2, 3, 1)
    Sx = _sigma_x(no[:, C:], C)
    al = alpha_b.view(B, 1, 1, 1)
    I, one = torch.eye(C, dtype=no.dtype), torch.ones(C, dtype=no.dtype)
    muy = 0.5 * al * one + (1 - al) * mu
    outer = lambda v: v[..., :, None] * v[..., None, :]         # noqa: E731
    Sy = al[..., None] * (I / 12 + 0.25 * outer(one)) + (1 - al[..., None]) * (Sx + outer(mu)) - outer(muy)
    d = yv - muy
    quad = (d[..., None, :] @ torch.linalg.solve(Sy, d[..., None]))[..., 0, 0]
    l = (0.5 * torch.logdet(Sy) + 0.5 * quad) * (2.0 if C == 1 else 1.0) - reg * al[..., 0]
    Sp = Sx + 1e-6 * I
    r = yv - mu
    f = torch.exp(-0.5 * (r[..., None, :] @ torch.linalg.solve(Sp, r[..., None]))[..., 0, 0]) / torch.sqrt((2 * math.pi) ** C * torch.linalg.det(Sp))
    f = f[..., None]
    pme = ((1 - al) * f * yv + al * mu) / ((1 - al) * f + al)
    return l.reshape(B, -1).mean(1), pme.permute(0, 3, 1, 2), no[:, :C]


def impulse_oracle(net_out, noisy, npar, mode, raw, w=None, g_pme=None, g_mu=None):
    """float64 autograd -> (outputs dict, dL/dnet_out, dL/d(raw: [1] or the var map), dL/dnoisy)"""
    B = net_out.shape[0]
    no = net_out.double().requires_grad_(True)
    y = noisy.double().requires_grad_(True)
    raw64 = None
    if mode == "known":
        alpha_b = npar.double().clamp(1e-3, 0.999)
    else:
        raw64 = raw.double().clone().requires_grad_(True)
        est = raw64.mean(dim=(1, 2, 3)) if mode == "var" else raw64.expand(B)
        alpha_b = (F.softplus(est - 4.0) + 1e-3).clamp(max=0.999)
    loss, pme, mu = impulse_forward_paper(no, y, alpha_b, 0.1 if mode != "known" else 0.0)
    L = 0
    if w is not None:
        L = L + (loss * w.double()).sum()
    if g_pme is not None:
        L = L + (pme * g_pme.double()).sum()
    if g_mu is not None:
        L = L + (mu * g_mu.double()).sum()
    leaves = [no, y] + ([raw64] if raw64 is not None else [])
    gs = torch.autograd.grad(L, leaves, allow_unused=True)
    gs = [torch.zeros_like(t) if g is None else g for g, t in zip(gs, leaves)]
    o = dict(loss=loss.detach(), pme=pme.detach(), mu=mu.detach(), alpha=alpha_b.detach())
    return o, gs[0], (gs[2] if raw64 is not None else None), gs[1]


def _close(a, b, rel, what=""):
    err = float((a - b).abs().max())
    scale = float(b.abs().max())
    assert err <= rel * scale + 1e-300, "%s: max abs err %.3e vs scale %.3e" % (what, err, scale)


def _est_raw(raw, mode):
    return raw.double().mean(dim=(1, 2, 3)) if mode == "var" else raw


# ---- 1. the mirror against autograd ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C", [1, 3])
def test_impulse_forward_vs_paper_form(C, mode, alpha):
    net_out, noisy, npar, raw = impulse_inputs(C, mode, alpha)
    B, H = net_out.shape[0], net_out.shape[2]
    wm = torch.full((B,), 1.0 / B)
    m = impulse_head(net_out, noisy, npar, mode, _est_raw(raw, mode), w=wm)
    o, g, graw, _ = impulse_oracle(net_out, noisy, npar, mode, raw, w=wm)
    _close(m["loss"], o["loss"], 1e-9, "loss")
    _close(m["pme"], o["pme"], 1e-9, "pme")
    _close(m["mu"], o["mu"], 0, "mu")
    _close(m["alpha"], o["alpha"], 1e-12, "alpha")
    assert float(m["model_std"][0, 1, 2]) == 0.0                    # all of A zero: a singular Sigma_x
    assert float((m["pme"][0, :, 1, 2] - m["mu"][0, :, 1, 2]).abs().max()) == 0.0         # ... whose pixel is certainly replaced
    _close(m["g_net_out"], g, 1e-9, "dL/dnet_out of mean(LOSS)")
    if mode == "const":
        _close(m["g_est"], graw.reshape(1), 1e-9, "g_est")
    if mode == "var":
        _close(m["g_est"].view(B, 1, 1, 1).expand_as(graw) / (H * H), graw, 1e-9, "g_sigma_out")


@pytest.mark.parametrize("terms", TERMS)
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C", [1, 3])
def test_impulse_vjp_and_noisy_grad_vs_autograd(C, mode, alpha, terms):
    net_out, noisy, npar, raw = impulse_inputs(C, mode, alpha, seed=1)
    B, H = net_out.shape[0], net_out.shape[2]
    g = torch.Generator().manual_seed(11)
    f = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    w = f(B) if terms in ("all", "loss") else None
    gp = f(B, C, H, H) if terms in ("all", "pme") else None
    gm = f(B, C, H, H) if terms in ("all", "mu") else None
    m = impulse_head(net_out, noisy, npar, mode, _est_raw(raw, mode), w, gp, gm)
    _, og, oraw, ody = impulse_oracle(net_out, noisy, npar, mode, raw, w, gp, gm)
    _close(m["g_net_out"], og, 1e-9, "dL/dnet_out")
    if terms != "mu":
        _close(m["g_noisy"], ody, 1e-9, "dL/dnoisy")
    else:
        assert float(m["g_noisy"].abs().max()) == 0.0 and float(ody.abs().max()) == 0.0
    if mode == "const":
        _close(m["g_est"], oraw.reshape(1), 1e-9, "g_est")
    if mode == "var":
        _close(m["g_est"].view(B, 1, 1, 1).expand_as(oraw) / (H * H), oraw, 1e-9, "g_sigma_out")


def test_impulse_alpha_clamp_has_zero_gradient():
    net_out, noisy, npar, _ = impulse_inputs(3, "const", 0.5)
    m = impulse_head(net_out, noisy, npar, "const", torch.full((1,), 9.0), w=torch.full((2,), 0.5))      # softplus(5) + 1e-3 > 0.999
    assert float(m["alpha"][0]) == 0.999 and float(m["g_est"].abs().max()) == 0.0
    assert torch.isfinite(m["g_net_out"]).all()


# ---- 2. / 3. synthetic draws ------------------------------------------------------------------------------------------------------------------
def _synthetic(alpha, seed):
    """x ~ N(mu, Sigma_x) per pixel, corrupted with alpha; the true (mu, A) as net_out"""
    g = torch.Generator().manual_seed(seed)
    B, S = 4, 64
    mu = 0.2 + 0.6 * torch.rand((B, 3, S, S), generator=g, dtype=torch.float64)
    A = -0.12 + 0.24 * torch.rand((B, 6, S, S), generator=g, dtype=torch.float64)
    z = torch.randn((B, 3, S, S), generator=g, dtype=torch.float64)
    x = torch.stack([mu[:, 0] + A[:, 0] * z[:, 0] + A[:, 1] * z[:, 1] + A[:, 2] * z[:, 2],       # mu + U z, U upper triangular
                     mu[:, 1] + A[:, 3] * z[:, 1] + A[:, 4] * z[:, 2], mu[:, 2] + A[:, 5] * z[:, 2]], 1)
    y, a = noise.add_impulse(x, alpha, generator=g)
    assert a == alpha
    return torch.cat([mu, A], 1), x, y


@pytest.mark.parametrize("alpha", [0.1, 0.5])
def test_impulse_posterior_mean_beats_the_noisy_pixel_and_the_prior(alpha):
    net_out, x, y = _synthetic(alpha, 5)
    m = impulse_head(net_out, y, torch.full((4,), alpha), "known", None)
    mse = lambda t: float(((t - x) ** 2).mean())     # noqa: E731
    e_pme, e_y, e_mu = mse(m["pme"]), mse(y), mse(net_out[:, :3])
    print("alpha %.1f: MSE posterior mean %.4f, noisy %.4f, prior mean %.4f" % (alpha, e_pme, e_y, e_mu))
    assert e_pme < e_y and e_pme < e_mu


@pytest.mark.parametrize("alpha", [0.1, 0.5])
def test_impulse_loss_gradient_has_zero_mean_at_the_true_parameters(alpha):
    net_out, x, y = _synthetic(alpha, 6)
    B, _, S, _ = net_out.shape
    m = impulse_head(net_out, y, torch.full((B,), alpha), "known", None, w=torch.full((B,), float(S * S)))     # per-pixel dl/dnet_out
    g = m["g_net_out"].permute(1, 0, 2, 3).reshape(9, -1)
    se = g.std(1) / math.sqrt(g.shape[1])
    ratio = (g.mean(1) / se).abs()
    print("alpha %.1f: |mean| / standard error per channel: %s" % (alpha, ["%.2f" % v for v in ratio.tolist()]))
    assert float(ratio.max()) <= 4.0


# ---- 4. the host data layer -----------------------------------------------------------------------------------------------------------------------
def test_impulse_style_grammar():
    assert noise.parse_style("impulse50") == ("impulse", [50], True)
    assert noise.parse_style("impulse0.25") == ("impulse", [0.25], True)
    assert noise.parse_style("impulse10_60") == ("impulse", [10, 60], True)
    assert noise.parse_style("impulse0.1_0.6_nc") == ("impulse", [0.1, 0.6], False)
    assert noise.impulse_alpha(50) == 0.5 and noise.impulse_alpha(0.25) == 0.25
    with pytest.raises(ValueError):
        noise.add_style(torch.zeros(3, 8, 8), "impulse150")


def _u8_images(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, shape, generator=g).float() / 255.0


def _check_impulse(x, y, alpha, ch_axis):
    """untouched pixels bit-equal, all channels or none, the replaced fraction and the replaced values' moments"""
    changed = y != x
    any_c, all_c = changed.any(ch_axis), changed.all(ch_axis)
    # (a drawn colour equals its 8-bit clean value in one channel with probability ~ 2^-24 * 256: not in these sizes)
    assert torch.equal(any_c, all_c), "a pixel is replaced in all channels or in none"
    assert torch.equal(y[~changed], x[~changed])
    n = any_c.numel()
    frac = float(any_c.float().mean())
    assert abs(frac - alpha) <= 5 * math.sqrt(alpha * (1 - alpha) / n), (frac, alpha)
    vals = y[changed].double()
    assert abs(float(vals.mean()) - 0.5) <= 5 * math.sqrt(1 / 12 / vals.numel())
    assert abs(float(vals.var()) - 1 / 12) <= 5 * math.sqrt(1 / 180 / vals.numel())        # Var((u - 1/2)^2) = 1/180
    assert 0.0 <= float(y.min()) and float(y.max()) <= 1.0
    return any_c


def test_add_impulse_chw_and_bchw():
    g = torch.Generator().manual_seed(3)
    x = _u8_images((3, 128, 128), 1)
    y, a = noise.add_style(x, "impulse50", generator=g)
    assert a == 0.5 and not torch.equal(x, y) and torch.equal(x, _u8_images((3, 128, 128), 1))          # not in place
    _check_impulse(x, y, 0.5, 0)
    xb = _u8_images((6, 3, 64, 64), 2)
    yb, a = noise.add_style(xb, "impulse0.2_nc", generator=g)
    assert a == 0.2
    _check_impulse(xb, yb, 0.2, 1)
    y1, _ = noise.add_impulse(_u8_images((1, 64, 64), 4), 0.3, generator=g)                                # mono
    _check_impulse(_u8_images((1, 64, 64), 4), y1, 0.3, 0)
    # in place
    z = x.clone()
    out, _ = noise.add_impulse(z, [50], inplace=True, generator=g)
    assert out.data_ptr() == z.data_ptr() and not torch.equal(z, x)


def test_add_impulse_ranged_is_one_alpha_per_image_and_reproducible():
    xb = _u8_images((8, 3, 64, 64), 7)
    yb, a = noise.add_style(xb, "impulse10_60", generator=torch.Generator().manual_seed(9))
    assert tuple(a.shape) == (8, 1, 1, 1) and float(a.min()) >= 0.1 and float(a.max()) < 0.6 and len(set(a.flatten().tolist())) == 8
    for b in range(8):
        mask = (yb[b] != xb[b]).any(0)
        al = float(a[b])
        assert abs(float(mask.float().mean()) - al) <= 5 * math.sqrt(al * (1 - al) / mask.numel())
        assert torch.equal((yb[b] != xb[b]).all(0), mask)
    x = _u8_images((3, 64, 64), 8)
    y, a = noise.add_style(x, "impulse10_60", generator=torch.Generator().manual_seed(9))
    assert tuple(a.shape) == (1, 1, 1)                                  # ONE draw for a CHW image, not one per channel
    y2, a2 = noise.add_style(x, "impulse10_60", generator=torch.Generator().manual_seed(9))
    assert torch.equal(y, y2) and torch.equal(a, a2)
    y3, _ = noise.add_style(x, "impulse10_60", generator=torch.Generator().manual_seed(10))
    assert not torch.equal(y, y3)


class _Patches(torch.utils.data.Dataset):
    def __init__(self, n=16, P=32, seed=3):
        self.x = _u8_images((n, 3, P, P), seed)

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return self.x[i], i


@pytest.mark.parametrize("alg", list(NoiseAlgorithm))
@pytest.mark.parametrize("style", ["impulse50", "impulse20_70"])
def test_impulse_noisy_dataset_and_device_stream_on_cpu(alg, style):
    from torch.utils.data import DataLoader
    from ssdn.datasets import CleanPatches, DevicePatchStream, NoisyDataset
    MD = NoisyDataset.Metadata
    torch.manual_seed(13)
    ds = NoisyDataset(_Patches(), style, alg, pad_uniform=False, pad_multiple=32, square=True, training_mode=True)
    host = next(iter(DataLoader(ds, batch_size=8, shuffle=False)))
    stream = DevicePatchStream(DataLoader(CleanPatches(ds), batch_size=8, shuffle=False), ds, "cpu", seed=5)
    dev = next(iter(stream))
    n2v = alg == NoiseAlgorithm.NOISE_TO_VOID
    for name, (inp, ref, md) in (("host", host), ("stream", dev)):
        clean = md[MD.CLEAN]
        assert inp.shape == clean.shape == (8, 3, 32, 32) and inp.dtype == torch.float32
        ch = inp != clean
        if not n2v:                                     # (Noise2Void copies neighbours into 16 pixels per image afterwards)
            assert torch.equal(ch.any(1), ch.all(1)), name
            assert torch.equal(inp[~ch], clean[~ch]), name
        a = md[MD.INPUT_NOISE_VALUES]
        frac = ch.any(1).float().mean(dim=(1, 2))
        if style == "impulse50":
            assert torch.allclose(a.flatten(), torch.full_like(a.flatten(), 0.5)), name
            assert float((frac - 0.5).abs().max()) <= 5 * math.sqrt(0.25 / 1024) + 16 / 1024, name
        else:
            assert float(a.min()) >= 0.2 and float(a.max()) < 0.7, name
            per = a.reshape(8, -1)
            assert bool((per == per[:, :1]).all()) and len(set(per[:, 0].tolist())) > 1, name          # one alpha per sample
            tol = 5 * (per[:, 0] * (1 - per[:, 0]) / 1024).sqrt() + 16 / 1024
            assert bool(((frac - per[:, 0]).abs() <= tol).all()), name
        if alg == NoiseAlgorithm.NOISE_TO_CLEAN:
            assert torch.equal(ref, clean)
        elif alg in (NoiseAlgorithm.NOISE_TO_NOISE, NoiseAlgorithm.NOISE_TO_VOID):
            cr = ref != clean
            assert torch.equal(cr.any(1), cr.all(1)) and not torch.equal(ref, inp), name
        elif alg == NoiseAlgorithm.SELFSUPERVISED_DENOISING_MEAN_ONLY:
            assert torch.equal(ref, inp)
        if n2v:
            assert tuple(md[MD.MASK_COORDS].shape) == (8, 16, 2)
    assert set(host[2].keys()) == set(dev[2].keys())
    for k in host[2]:
        if style == "impulse50" or k not in (MD.INPUT_NOISE_VALUES, MD.REFERENCE_NOISE_VALUES):
            assert host[2][k].shape == dev[2][k].shape and host[2][k].dtype == dev[2][k].dtype, k


# ---- 5. plumbing that needs no GPU ------------------------------------------------------------------------------------------------------------------
def test_impulse_engine_style_and_abi():
    from ssdn.hip import lib as L
    from ssdn.hip.engine import STYLE, engine_style
    assert STYLE == {"gauss": 0, "poisson": 1, "impulse": 2}
    assert engine_style("impulse50") == "impulse" and engine_style("impulse10_60_nc") == "impulse"
    assert engine_style("gauss25") == "gauss" and engine_style("poisson30") == "poisson" and engine_style("speckle3") == "gauss"
    assert L.ABI_VERSION == 19


def test_impulse_denoiser_config_round_trip(tmp_path):
    d = Denoiser(impulse_cfg("impulse50", "const"), device="cpu")
    assert "impulse50" in d.config_name()
    assert d.state_dict()["_models.denoiser_model.output_block.4.bias"].shape == (9,)
    torch.save(d.state_dict(), tmp_path / "run.training")
    back = Denoiser.from_state_dict(torch.load(tmp_path / "run.training", weights_only=False))
    assert back.cfg[ConfigValue.NOISE_STYLE] == "impulse50" and back.config_name() == d.config_name()
    with pytest.raises(NotImplementedError, match="impulse"):
        Denoiser(impulse_cfg("impulse50", "known", diag=True), device="cpu")
    Denoiser(impulse_cfg("gauss25", "known", diag=True), device="cpu")              # (the flag alone is fine)


def test_cli_train_start_impulse_builds_the_model(tmp_path, monkeypatch):
    from ssdn.cli.cli import build_parser
    from ssdn.train import DenoiserTrainer
    built = {}

    def fake_train(self):            # (the run itself needs a GPU: stop where the model has been built)
        self.new_target()
        built["trainer"] = self

    monkeypatch.setattr(DenoiserTrainer, "train", fake_train)
    parser, cmds = build_parser()
    h5 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g_libhdf5_dataset.h5")
    args = vars(parser.parse_args(["train", "start", "-a", "ssdn", "-n", "impulse50", "--noise_value", "const", "-t", h5,
                                   "-i", "1000", "--runs_dir", str(tmp_path)]))
    args["PARSER"] = parser
    cmds["train"].execute(args)
    tr = built["trainer"]
    assert tr.cfg[ConfigValue.NOISE_STYLE] == "impulse50"
    d = tr.denoiser
    assert "impulse50" in d.config_name()
    assert d.state_dict()["_models.denoiser_model.output_block.4.weight"].shape == (9, 96, 1, 1)
