"""CPU: the closed forms of the loss head's direct input term (SSDN_OP_HEAD_VJP's g_noisy), restated in float64
torch, against float64 autograd of the oracle head (oracle/restate.py) with respect to the noisy image, net_out and the noise level held
fixed.  The GPU tests (tests/test_hip_denoiser_input_grad.py) reuse `head_dy64`."""
import itertools

import pytest
import torch

import restate as R
from test_head_vjp_cpu import VARIANTS, head_inputs, upstream

TERMS = [t for n in (1, 2, 3) for t in itertools.combinations(("loss", "pme", "mu"), n)]


def _sigma64(no, npar, style, mode, est_raw, C):
    """per-channel sigma [B,C,H,W] as the head computes it (float64)"""
    B, _, H, W = no.shape
    mu = no[:, :C]
    npar = npar.double().view(B, 1, 1, 1)
    if mode != "known":
        raw = est_raw.double().reshape(-1)
        est = (torch.nn.functional.softplus(raw - 4.0) + 1e-3).expand(B).reshape(B, 1, 1, 1)
    if style.startswith("gauss"):
        return (npar.clamp(min=1e-3) if mode == "known" else est).expand(B, C, H, W)
    f = 1.0 / npar if mode == "known" else est
    return (mu.clamp(min=1e-3) * f).sqrt()


def head_dy64(net_out, noisy, npar, style, mode, est_raw, w=None, g_pme=None, g_mu=None):
    """dL/dnoisy of the head alone (net_out and sigma fixed), the kernel's closed forms in float64.  est_raw: [1] (const) or [B] (var)
    pre-softplus values.  g_mu does not enter: mu does not depend on the noisy image."""
    no, y = net_out.double(), noisy.double()
    B, _, H, W = no.shape
    C = y.shape[1]
    sc = (w.double() if w is not None else torch.zeros(B, dtype=torch.float64)).view(B, 1, 1, 1) / (H * W)
    mu = no[:, :C]
    sig = _sigma64(no, npar, style, mode, est_raw, C)
    d = y - mu
    if C == 1:
        sx, sn = no[:, 1:2] ** 2, sig ** 2
        sy = sx + sn
        gy = 2 * sc * d / sy                              # l = d^2/sy + log sy
        if g_pme is not None:                             # pme = (y sx + mu sn) / sy
            gy = gy + g_pme.double() * sx / sy
        return gy
    A = no[:, 3:].permute(0, 2, 3, 1)
    U = torch.zeros(B, H, W, 3, 3, dtype=torch.float64)
    for k, (i, j) in enumerate([(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]):
        U[..., i, j] = A[..., k]
    Sx = U @ U.transpose(-1, -2)
    Sy = Sx + torch.diag_embed((sig ** 2).permute(0, 2, 3, 1))
    dv = d.permute(0, 2, 3, 1)[..., None]
    gy = torch.linalg.inv(Sy) @ dv * sc.view(B, 1, 1, 1, 1)       # l = 1/2 d^T Sy^-1 d + 1/2 log det Sy: no factor 2
    if g_pme is not None:                                          # pme = mu + S' T^-1 d: h = T^-1 S' g
        eye = torch.eye(3, dtype=torch.float64)
        gv = g_pme.double().permute(0, 2, 3, 1)[..., None]
        gy = gy + torch.linalg.inv(Sy + 2e-6 * eye) @ ((Sx + 1e-6 * eye) @ gv)
    return gy[..., 0].permute(0, 3, 1, 2)


def pme_kernel_form64(net_out, noisy, sig):
    """the 3-channel posterior mean in the kernel's form mu + S' T^-1 (y - mu) (k_head), float64, differentiable"""
    B, _, H, W = net_out.shape
    A = net_out[:, 3:].permute(0, 2, 3, 1)
    z = torch.zeros_like(A[..., 0])
    U = torch.stack([torch.stack([A[..., 0], A[..., 1], A[..., 2]], -1), torch.stack([z, A[..., 3], A[..., 4]], -1),
                     torch.stack([z, z, A[..., 5]], -1)], -2)
    Sx = U @ U.transpose(-1, -2)
    eye = torch.eye(3, dtype=torch.float64)
    T = Sx + torch.diag_embed((sig ** 2).permute(0, 2, 3, 1)) + 2e-6 * eye
    mu = net_out[:, :3].permute(0, 2, 3, 1)[..., None]
    d = noisy.permute(0, 2, 3, 1)[..., None] - mu
    return (mu + (Sx + 1e-6 * eye) @ torch.linalg.solve(T, d))[..., 0].permute(0, 3, 1, 2)


def oracle_dy(net_out, noisy, npar, style, mode, raw, w, g_pme, g_mu, kernel_pme=False):
    """float64 autograd of R.ssdn_head with respect to `noisy` alone.  kernel_pme: the posterior-mean term through the kernel's form
    (pme_kernel_form64) instead of the reference's (Sx'^-1 + Sn'^-1 + eps I)^-1 (Sx'^-1 mu + Sn'^-1 y), which agrees with it only up to
    the eps terms"""
    B, C = noisy.shape[:2]
    y = noisy.double().requires_grad_(True)
    est = None
    if raw is not None:
        est = raw.double().reshape((B, 1) + tuple(raw.shape[2:]) if mode == "var" else (1, 1, 1, 1))
        est = est.mean(dim=(2, 3), keepdim=True) if mode == "var" else est
    o = R.ssdn_head(net_out.double(), y, npar.double().view(B, 1, 1, 1), style, mode, est)
    L = 0
    if w is not None:
        L = L + (o["loss"].view(B) * w.double()).sum()
    if g_pme is not None:
        pme = o["out"]
        if kernel_pme and C == 3:
            est_raw = raw.double().mean(dim=(1, 2, 3)) if mode == "var" else raw
            pme = pme_kernel_form64(net_out.double(), y, _sigma64(net_out.double(), npar, style, mode, est_raw, C))
        L = L + (pme * g_pme.double()).sum()
    if g_mu is not None:
        L = L + (o["out_mu"] * g_mu.double()).sum()
    if not torch.is_tensor(L) or not L.requires_grad:
        return torch.zeros_like(y)
    L.backward()
    return y.grad if y.grad is not None else torch.zeros_like(y)


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize("ch,style,mode", VARIANTS)
@pytest.mark.parametrize("terms", TERMS, ids=["+".join(t) for t in TERMS])
def test_head_input_term_closed_forms_vs_autograd(ch, style, mode, terms):
    net_out, noisy, npar, raw = head_inputs(ch, style, mode)
    B, H = net_out.shape[0], net_out.shape[2]
    w, gp, gm = upstream(B, ch, H, seed=17 + ch, w="loss" in terms, g_pme="pme" in terms, g_mu="mu" in terms)
    est_raw = raw.double().mean(dim=(1, 2, 3)) if mode == "var" else raw
    got = head_dy64(net_out, noisy, npar, style, mode, est_raw, w, gp, gm)
    if terms == ("mu",):
        assert torch.count_nonzero(got) == 0                       # mu does not read the noisy image
        assert torch.count_nonzero(oracle_dy(net_out, noisy, npar, style, mode, raw, w, gp, gm)) == 0
        return
    # against the kernel's own posterior-mean form: rounding only
    want = oracle_dy(net_out, noisy, npar, style, mode, raw, w, gp, gm, kernel_pme=True)
    assert _rel(got, want) <= 1e-9, _rel(got, want)
    # against the reference's form: for C = 1 and without a 3-channel posterior-mean term, the same expression (rounding only); the
    # 3-channel posterior mean differs from the reference's by its eps terms -- the bound of test_head_vjp_cpu.py
    ref = oracle_dy(net_out, noisy, npar, style, mode, raw, w, gp, gm)
    assert _rel(got, ref) <= (1e-5 if ch == 3 and "pme" in terms else 1e-9), _rel(got, ref)
