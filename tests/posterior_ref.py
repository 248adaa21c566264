"""The per-pixel posterior of SSDN_OP_HEAD_POSTERIOR (csrc/head_posterior.hip) as a torch mirror: the kernel's formulas, operation by
operation, in float64 (the reference of the tests) or in fp32 (what the number format alone costs on the same inputs).  Helpers the CPU
and GPU tests share: the inputs of the op cases, the symmetric 3x3 matrix of a Sym3-ordered tensor, the fp32 yardstick."""
import math

import torch
import torch.nn.functional as F

import restate as R
from test_diag_cov_cpu import NPAR, diag_inputs
from test_impulse_cpu import _sym_adj, _sym_mv, impulse_inputs

EPS = 1e-6
TRI = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))        # the Sym3 order of `cov`


def is_impulse(style):
    return style.startswith("impulse")


def _est(mode, est_raw, B, dtype):
    raw = est_raw.to(dtype).reshape(-1)
    raw = raw.expand(B) if raw.numel() == 1 else raw
    return (F.softplus(raw - 4.0) + 1e-3).view(B, 1, 1)


def _sigma(style, mode, npar, est, mu):
    """head_sigma: sigma_c [B,H,W] of one channel"""
    if style.startswith("gauss"):
        return (npar.clamp(min=1e-3) if mode == "known" else est).expand_as(mu)
    m = mu.clamp(min=1e-3)
    return (m * (1.0 / npar if mode == "known" else est)).sqrt()


def posterior_ref(net_out, noisy, npar, style, mode, est_raw, diag=0, dtype=torch.float64):
    """-> dict: mean [B,C,H,W], cov [B,C(C+1)/2,H,W] (Sym3 order), std [B,C,H,W]; impulse also w [B,H,W] (P(untouched | y)) and the prior's
    mu_x / Sigma_x (`prior_mean`, `prior_cov`).  est_raw: [1] (const) or [B] (var), pre-softplus; npar [B]."""
    no, y = net_out.to(dtype), noisy.to(dtype)
    B, Cout, H, W = no.shape
    C = y.shape[1]
    mu = [no[:, c] for c in range(C)]
    A = [no[:, C + c] for c in range(Cout - C)]
    yy = [y[:, c] for c in range(C)]
    out = {}
    if is_impulse(style):
        assert not diag
        if mode == "known":
            alpha = npar.to(dtype).reshape(B).clamp(1e-3, 0.999)
        else:
            alpha = _est(mode, est_raw, B, dtype).view(B).clamp(max=0.999)
        al = alpha.view(B, 1, 1)
        lodds = torch.log(1 - al) - torch.log(al)
        r = [yy[c] - mu[c] for c in range(C)]
        if C == 1:
            sx = A[0] * A[0]
            sp = sx + 1e-6
            t = r[0] * (1 / sp)
            z = lodds - 0.5 * torch.log(sp) - 0.5 * r[0] * t - 0.5 * math.log(2 * math.pi)
            x = [sx]
        else:
            x = [A[0] * A[0] + A[1] * A[1] + A[2] * A[2], A[1] * A[3] + A[2] * A[4], A[2] * A[5], A[3] * A[3] + A[4] * A[4], A[4] * A[5],
                 A[5] * A[5]]
            sp = (x[0] + 1e-6, x[1], x[2], x[3] + 1e-6, x[4], x[5] + 1e-6)
            cp, detp = _sym_adj(sp)
            detp = detp.clamp(min=1e-18)
            t = _sym_mv(cp, r, 1 / detp)
            quad = (r[0] * t[0] + r[1] * t[1] + r[2] * t[2]).clamp(min=0)
            z = lodds - 0.5 * torch.log(detp) - 0.5 * quad - 1.5 * math.log(2 * math.pi)
        w, wm = torch.sigmoid(z), torch.sigmoid(-z)
        ij = TRI if C == 3 else ((0, 0),)
        cov = [wm * x[n] + (w * wm) * (r[i] * r[j]) for n, (i, j) in enumerate(ij)]
        mean = [mu[c] + w * r[c] for c in range(C)]
        out.update(w=w, prior_mean=torch.stack(mu, 1), prior_cov=torch.stack(x, 1))
    else:
        npv = npar.to(dtype).view(B, 1, 1)
        est = _est(mode, est_raw, B, dtype) if mode != "known" else None
        sig = [_sigma(style, mode, npv, est, mu[c]) for c in range(C)]
        n = [s * s for s in sig]
        if C == 1:
            sx = A[0] * A[0]
            sy = sx + n[0]
            cov = [sx * n[0] / sy]
            mean = [(yy[0] * sx + mu[0] * n[0]) / sy]
        elif diag:
            zero = torch.zeros_like(mu[0])
            cov, mean = [zero] * 6, []
            for c in range(3):
                ix, iN = 1 / (A[c] * A[c] + EPS), 1 / (n[c] + EPS)
                rD = 1 / (ix + iN + EPS)
                cov[(0, 3, 5)[c]] = rD
                mean.append(mu[c] * (ix * rD) + yy[c] * (iN * rD))
        else:
            x = [A[0] * A[0] + A[1] * A[1] + A[2] * A[2], A[1] * A[3] + A[2] * A[4], A[2] * A[5], A[3] * A[3] + A[4] * A[4], A[4] * A[5],
                 A[5] * A[5]]
            t = ((x[0] + n[0]) + 2 * EPS, x[1], x[2], (x[3] + n[1]) + 2 * EPS, x[4], (x[5] + n[2]) + 2 * EPS)
            k, det = _sym_adj(t)
            rd = 1 / det
            d = [yy[c] - mu[c] for c in range(3)]
            q = _sym_mv(k, d, rd)
            xp = (x[0] + EPS, x[3] + EPS, x[5] + EPS)
            X = [[xp[0], x[1], x[2]], [x[1], xp[1], x[4]], [x[2], x[4], xp[2]]]
            Kf = [[k[0], k[1], k[2]], [k[1], k[3], k[4]], [k[2], k[4], k[5]]]
            mean = [mu[i] + X[i][0] * q[0] + X[i][1] * q[1] + X[i][2] * q[2] for i in range(3)]
            g = [[X[i][0] * Kf[0][j] + X[i][1] * Kf[1][j] + X[i][2] * Kf[2][j] for j in range(3)] for i in range(3)]
            m = [(n[c] + EPS) * rd for c in range(3)]
            cov = [g[i][j] * m[j] if i == j else 0.5 * (g[i][j] * m[j] + g[j][i] * m[i]) for (i, j) in TRI]
    cov = torch.stack(cov, 1)
    dg = cov if C == 1 else cov[:, [0, 3, 5]]
    out.update(mean=torch.stack(mean, 1), cov=cov, std=dg.clamp(min=0).sqrt())
    return out


def full_matrix(tri):
    """[B,6,H,W] in Sym3 order (or [B,1,H,W]) -> [B,H,W,C,C]"""
    if tri.shape[1] == 1:
        return tri.permute(0, 2, 3, 1)[..., None]
    B, _, H, W = tri.shape
    m = torch.zeros((B, H, W, 3, 3), dtype=tri.dtype)
    for n, (i, j) in enumerate(TRI):
        m[..., i, j] = tri[:, n]
        m[..., j, i] = tri[:, n]
    return m


def est_of(raw, mode):
    """what the op takes as est_raw: the spatial mean of a var map, the scalar of const"""
    if raw is None:
        return None
    return raw.mean(dim=(1, 2, 3)) if mode == "var" else raw


def op_inputs(style, mode, C, diag=0, B=2, H=5, W=7, alpha=0.5, seed=0):
    """net_out, noisy, npar [B], est_raw of one op case, [B,*,H,W]: the inputs of the impulse / diagonal head tests (impulse_inputs,
    diag_inputs: means in (0.05, 0.95), A in (-0.4, 0.6), their zeroed / ill-conditioned pixels in the top-left corner), generated square at
    max(H, W, 8) with at least two batch elements and cropped.  The full Gaussian / Poisson heads take impulse_inputs' net_out and noisy
    with diag_inputs' noise parameters."""
    S, want_B, B = max(H, W, 8), B, max(B, 2)          # (the generators address batch element 1)
    if is_impulse(style):
        no, y, npar, raw = impulse_inputs(C, mode, alpha, B=B, H=S, seed=seed)
    elif diag and C == 3:
        no, y, npar, raw = diag_inputs(style, mode, B=B, H=S, seed=seed)
    else:
        no, y, _, _ = impulse_inputs(C, "known", 0.5, B=B, H=S, seed=seed)
        _, _, npar, raw = diag_inputs(style, mode, B=B, H=S, seed=seed)
    est = est_of(raw, mode)           # (the mean over the whole square map: any value serves)
    if est is not None and est.numel() > 1:
        est = est[:want_B]
    return no[:want_B, :, :H, :W].contiguous(), y[:want_B, :, :H, :W].contiguous(), npar[:want_B], est


def fp32_yardstick(net_out, noisy, npar, style, mode, est_raw, diag, m64):
    """the mirror in fp32 torch against float64, max abs error per output (impulse: of the weight `w` too): what the number format alone
    costs on these inputs"""
    m32 = posterior_ref(net_out, noisy, npar, style, mode, est_raw, diag, dtype=torch.float32)
    fig = {k: float((m32[k].double() - m64[k]).abs().max()) for k in ("mean", "cov", "std") + (("w",) if "w" in m64 else ())}
    print("fp32 mirror vs float64, max abs error: " + ", ".join("%s %.2e (max |.| %.2e)" % (k, v, float(m64[k].abs().max())) for k, v in fig.items()))
    return fig


__all__ = ["posterior_ref", "full_matrix", "op_inputs", "fp32_yardstick", "est_of", "is_impulse", "TRI", "EPS", "NPAR", "R"]
