"""CPU: the closed forms of the loss heads' vector-Jacobian product (SSDN_OP_HEAD_VJP / SSDN_OP_MSE_VJP),
restated in float64 torch, against autograd of the oracle (oracle/restate.py) for random upstream gradients of LOSS, the posterior mean
and mu.  The GPU tests (tests/test_hip_denoiser_autograd.py) reuse `head_vjp64` and `head_inputs`."""
import pytest
import torch
import torch.nn.functional as F

import restate as R

VARIANTS = [(ch, style, mode) for ch in (1, 3) for style in ("gauss25", "poisson30") for mode in ("known", "const", "var")]
NPAR = {"gauss25": 25 / 255.0, "poisson30": 30.0}


def head_inputs(ch, style, mode, B=2, H=8):
    """the well-conditioned inputs of tests/test_hip_head.py: net_out, noisy, noise parameter [B], raw estimate map (var: [B,1,H,W])
    or scalar (const), all float32"""
    ncomp = ch + ch * (ch + 1) // 2
    net_out = R.hash_tensor((B, ncomp, H, H), 41 + ch, -0.4, 0.6)
    net_out[:, :ch] = R.hash_tensor((B, ch, H, H), 42, 0.05, 0.95)
    noisy = R.hash_tensor((B, ch, H, H), 43, 0.0, 1.0)
    npar = torch.full((B,), NPAR[style])
    raw = None
    if mode == "var":
        raw = R.hash_tensor((B, 1, H, H), 44, 1.0, 3.0)
    elif mode == "const":
        raw = torch.full((1,), 1.7)
    return net_out, noisy, npar, raw


def upstream(B, ch, H, seed=0, w=True, g_pme=True, g_mu=True):
    g = torch.Generator().manual_seed(seed)
    f = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    return (f(B) if w else None), (f(B, ch, H, H) if g_pme else None), (f(B, ch, H, H) if g_mu else None)


def head_vjp64(net_out, noisy, npar, style, mode, est_raw, w=None, g_pme=None, g_mu=None):
    """The kernel's closed forms in float64.  est_raw: [1] (const) or [B] (var) pre-softplus values.
    -> (dL/dnet_out [B,Cout,H,W], dL/dest_raw: [1] const, [B] var, None known)"""
    d64 = lambda t: None if t is None else t.double()    # noqa: E731
    no, y = d64(net_out), d64(noisy)
    w, gp, gm = d64(w), d64(g_pme), d64(g_mu)
    B, _, H, W = no.shape
    C = y.shape[1]
    HW = H * W
    sc = (w if w is not None else torch.zeros(B, dtype=torch.float64)).view(B, 1, 1) / HW
    mu = no[:, :C]
    # sigma per channel and its derivatives (the head's dsig_dmu / dsig_dest)
    if mode != "known":
        raw = d64(est_raw).reshape(-1)
        raw = raw.expand(B) if raw.numel() == 1 else raw
        est, dest_draw = F.softplus(raw - 4.0) + 1e-3, torch.sigmoid(raw - 4.0)
        est, dest_draw = est.view(B, 1, 1, 1), dest_draw.view(B, 1, 1, 1)
    npar = d64(npar).view(B, 1, 1, 1)
    if style.startswith("gauss"):
        sig = (npar.clamp(min=1e-3) if mode == "known" else est).expand(B, C, H, W)
        dsig_dmu = torch.zeros_like(mu)
        dsig_dest = torch.ones_like(mu)
    else:
        m = mu.clamp(min=1e-3)
        f = 1.0 / npar if mode == "known" else est
        sig = (m * f).sqrt()
        dsig_dmu = torch.where(mu > 1e-3, 0.5 * f / sig, torch.zeros_like(mu))
        dsig_dest = 0.5 * m / sig
    reg = 0.1 if mode != "known" else 0.0
    d = y - mu
    if C == 1:
        sx, sn = no[:, 1:2] ** 2, sig ** 2
        sy = sx + sn
        sc4 = sc.view(B, 1, 1, 1)
        dsy = (-d * d / sy ** 2 + 1 / sy) * sc4
        dmu, dsx, dsn, dsig = -2 * d / sy * sc4, dsy.clone(), dsy.clone(), -reg * sc4
        if gp is not None:                                 # pme = (y sx + mu sn) / sy
            dmu = dmu + gp * sn / sy
            dsx = dsx + gp * sn * d / sy ** 2
            dsn = dsn - gp * sx * d / sy ** 2
        dsig = dsig + 2 * sig * dsn
        gmu = dmu + dsig * dsig_dmu + (gm if gm is not None else 0)
        g = torch.cat([gmu, 2 * no[:, 1:2] * dsx], 1)
    else:
        A = no[:, 3:].permute(0, 2, 3, 1)                  # [B,H,W,6]
        U = torch.zeros(B, H, W, 3, 3, dtype=torch.float64)
        iu = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
        for k, (i, j) in enumerate(iu):
            U[..., i, j] = A[..., k]
        Sx = U @ U.transpose(-1, -2)
        n = (sig ** 2).permute(0, 2, 3, 1)
        Sy = Sx + torch.diag_embed(n)
        dv = d.permute(0, 2, 3, 1)[..., None]              # [B,H,W,3,1]
        Si = torch.linalg.inv(Sy)
        q = Si @ dv
        sc5 = sc.view(B, 1, 1, 1, 1)
        G = (0.5 * Si * (torch.linalg.det(Sy) > 0)[..., None, None] - 0.5 * q @ q.transpose(-1, -2)) * sc5
        dn = torch.diagonal(G, dim1=-2, dim2=-1).clone()
        gmu = -q[..., 0] * sc5[..., 0]
        rg = reg / 3.0 * sc.view(B, 1, 1, 1)
        if gp is not None:                                 # pme = mu + S' T^-1 d
            eye = torch.eye(3, dtype=torch.float64)
            Sp = Sx + 1e-6 * eye
            Ti = torch.linalg.inv(Sy + 2e-6 * eye)
            gv = gp.permute(0, 2, 3, 1)[..., None]
            r = Ti @ dv
            h = Ti @ (Sp @ gv)
            e = gv - h
            gmu = gmu + e[..., 0]
            Gp = e @ r.transpose(-1, -2)
            G = G + 0.5 * (Gp + Gp.transpose(-1, -2))
            dn = dn - (h * r)[..., 0]
        ds = 2 * sig.permute(0, 2, 3, 1) * dn - rg
        gmu = gmu + ds * dsig_dmu.permute(0, 2, 3, 1)
        if gm is not None:
            gmu = gmu + gm.permute(0, 2, 3, 1)
        gU = 2 * G @ U                                     # dL/dU on the upper triangle (G symmetric, per-matrix-element convention)
        gA = torch.stack([gU[..., i, j] for i, j in iu], -1)
        g = torch.cat([gmu, gA], -1).permute(0, 3, 1, 2)
        dsig = ds.permute(0, 3, 1, 2)
    if mode == "known":
        return g, None
    gest = (dsig * dsig_dest).sum(dim=(1, 2, 3)) * dest_draw.view(B)
    return g, (gest.sum().view(1) if mode == "const" else gest)


def oracle_vjp(net_out, noisy, npar, style, mode, raw, w, g_pme, g_mu):
    """autograd of R.ssdn_head in float64: dL/dnet_out and dL/d(raw estimate: the scalar, or the var map [B,1,H,W])"""
    B = net_out.shape[0]
    C = noisy.shape[1]
    no = net_out.double().requires_grad_(True)
    raw64 = est64 = None
    if raw is not None:
        raw64 = raw.double().reshape((B, 1) + tuple(raw.shape[2:]) if mode == "var" else (1, 1, 1, 1)).requires_grad_(True)
        est64 = raw64.mean(dim=(2, 3), keepdim=True) if mode == "var" else raw64
    o = R.ssdn_head(no, noisy.double(), npar.double().view(B, 1, 1, 1), style, mode, est64)
    L = 0
    if w is not None:
        L = L + (o["loss"].view(B) * w.double()).sum()
    if g_pme is not None:
        L = L + (o["out"] * g_pme.double()).sum()
    if g_mu is not None:
        L = L + (o["out_mu"] * g_mu.double()).sum()
    L.backward()
    graw = None
    if raw64 is not None:
        graw = raw64.grad if raw64.grad is not None else torch.zeros_like(raw64)    # (mu alone does not depend on a gauss estimate)
    return no.grad, graw


def _close(a, b, rel):
    err = float((a - b).abs().max())
    scale = float(b.abs().max())
    assert err <= rel * scale, "max abs err %.3e vs scale %.3e" % (err, scale)


@pytest.mark.parametrize("ch,style,mode", VARIANTS)
@pytest.mark.parametrize("terms", ["all", "loss", "pme", "mu"])
def test_head_vjp_closed_forms_vs_autograd(ch, style, mode, terms):
    net_out, noisy, npar, raw = head_inputs(ch, style, mode)
    B, H = net_out.shape[0], net_out.shape[2]
    w, gp, gm = upstream(B, ch, H, seed=7 + ch, w=terms in ("all", "loss"), g_pme=terms in ("all", "pme"), g_mu=terms in ("all", "mu"))
    est_raw = raw.double().mean(dim=(1, 2, 3)) if mode == "var" else raw
    g, gest = head_vjp64(net_out, noisy, npar, style, mode, est_raw, w, gp, gm)
    og, oraw = oracle_vjp(net_out, noisy, npar, style, mode, raw, w, gp, gm)
    # the oracle's 3-channel posterior mean is the reference's (Sx'^-1 + Sn'^-1 + eps I)^-1 (...) form, the kernel's mu + S' T^-1 d:
    # algebraically equal up to the eps terms
    _close(g, og, 1e-6 if ch == 1 or terms in ("loss", "mu") else 1e-5)
    if mode == "const":
        _close(gest, oraw.reshape(1), 1e-6 if ch == 1 else 1e-5)
    if mode == "var":
        _close(gest.view(B, 1, 1, 1).expand_as(oraw) / (H * H), oraw, 1e-6 if ch == 1 else 1e-5)


def mse_vjp64(out, ref, w, g_pme, coords=None):
    """g = w[b] dLOSS[b]/dout + g_pme; masked: batch element 0's coordinates for every element, duplicates counted"""
    out, ref = out.double(), ref.double()
    B, C, H, W = out.shape
    g = torch.zeros_like(out)
    if w is not None:
        wb = w.double().view(B, 1, 1, 1)
        if coords is None:
            g = g + wb * 2 * (out - ref) / (C * H * W)
        else:
            for r, c in coords[0].tolist():
                g[:, :, r, c] += (wb * 2 * (out - ref) / C)[:, :, r, c]
    if g_pme is not None:
        g = g + g_pme.double()
    return g


@pytest.mark.parametrize("masked", [False, True])
def test_mse_vjp_closed_forms_vs_autograd(masked):
    B, C, H = 3, 3, 16
    out = R.hash_tensor((B, C, H, H), 51, 0, 1)
    ref = R.hash_tensor((B, C, H, H), 52, 0, 1)
    w, gp, _ = upstream(B, C, H, seed=3, g_mu=False)
    coords = None
    if masked:
        k = torch.Generator().manual_seed(5)
        c0 = torch.randint(0, H, (12, 2), generator=k)
        c0[5] = c0[2]                                     # a duplicate coordinate counts twice
        c0[9] = c0[2]
        coords = torch.stack([c0, torch.randint(0, H, (12, 2), generator=k)])    # element 1's coordinates are ignored
    for ww, gg in ((w, gp), (w, None), (None, gp)):
        o = out.double().requires_grad_(True)
        loss = R.mask_mse_loss(coords, o, ref.double()) if masked else R.mse_loss(o, ref.double())
        L = 0
        if ww is not None:
            L = L + (loss.view(B) * ww.double()).sum()
        if gg is not None:
            L = L + (o * gg.double()).sum()
        L.backward()
        _close(mse_vjp64(out, ref, ww, gg, coords), o.grad, 1e-12)
