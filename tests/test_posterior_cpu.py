"""CPU: the per-pixel posterior (SSDN_OP_HEAD_POSTERIOR, Denoiser.posterior, `ssdn eval --posterior`): the C ABI and its argument rules
(raised before any device call, so they show without a GPU), the float64 mirror of the kernel's formulas (tests/posterior_ref.py) against
independent formulations, its calibration on data drawn from the model, and the interface's refusals."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import restate as R
import ssdn
from ssdn.denoiser import Denoiser
from ssdn.hip import lib as L
from ssdn.params import ConfigValue, NoiseAlgorithm
from posterior_ref import EPS, NPAR, full_matrix, op_inputs, posterior_ref
from test_diag_cov_cpu import diag_cfg, scatter9
from test_impulse_cpu import impulse_head, impulse_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GP_CASES = [(style, mode, C) for style in ("gauss25", "poisson30") for mode in ("known", "const", "var") for C in (1, 3)]


# ---- 1. the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_struct_size():
    hdr = open(os.path.join(ROOT, "include", "ssdn_hip.h")).read()
    assert re.search(r"SSDN_OP_HEAD_POSTERIOR\s*=\s*26\b", hdr) and "} ssdn_head_posterior_args;" in hdr
    assert L.OP["head_posterior"] == 26 and L.ARG_TYPES["head_posterior"] is L.HeadPosteriorArgs
    assert [n for n, _ in L.HeadPosteriorArgs._fields_] == ["net_out", "noisy", "noise_param", "est_raw", "B", "C", "H", "W", "style", "mode",
                                                            "diag", "nchunks", "cov", "std", "samples", "n_samples", "seed", "offset"]
    assert L.load().ssdn_struct_size(26) == C.sizeof(L.HeadPosteriorArgs) == 112


def _refused(**kw):
    """run one op with dummy (never dereferenced) pointers -> the library's error text"""
    f = dict(net_out=0x1000, noisy=0x1000, noise_param=0x1000, est_raw=None, B=1, C=3, H=2, W=2, style=0, mode=0, diag=0, nchunks=1,
             cov=0x1000, std=None, samples=None, n_samples=0, seed=0, offset=0)
    f.update(kw)
    a = L.HeadPosteriorArgs(**f)
    rec = (L.OpRec * 1)()
    rec[0].type, rec[0].lane, rec[0].args = L.OP["head_posterior"], 0, C.cast(C.pointer(a), C.c_void_p)
    lib = L.load()
    assert lib.ssdn_run_ops(rec, 1, None) != 0
    return lib.ssdn_last_error().decode()


@pytest.mark.parametrize("kw,msg", [
    (dict(C=2), "C must be 1 or 3"),
    (dict(style=2, diag=1), r"style 2 \(impulse\) with diag = 1 \(DIAGONAL_COVARIANCE\) is not supported"),
    (dict(cov=None), "one of cov, std and samples must be given"),
    (dict(samples=0x1000, n_samples=0), "samples needs n_samples >= 1"),
    (dict(noise_param=None), "mode known needs noise_param"),
    (dict(mode=1), "modes const / var need est_raw"),
    (dict(B=1 << 20, H=1 << 10, W=1 << 10), r"B H W must be below 2\^32"),
])
def test_run_ops_refuses_bad_arguments_without_a_gpu(kw, msg):
    err = _refused(**kw)
    assert re.search(r"head_posterior: " + msg, err), err


def test_impulse_diag_refusal_uses_the_heads_words():
    src = open(os.path.join(ROOT, "selfsupervised-denoising_amd", "csrc", "head_impulse.hip")).read()
    words = "style 2 (impulse) with diag = 1 (DIAGONAL_COVARIANCE) is not supported"
    assert 'head: ' + words in src and _refused(style=2, diag=1).endswith("head_posterior: " + words)


# ---- 2. the mirror against independent formulations -----------------------------------------------------------------------------------------
def _sx_sn(no, style, mode, npar, est_raw):
    """Sigma_x, Sigma_n [B,H,W,3,3] in float64, written with matrices (not the kernel's scalars)"""
    no = no.double()
    B = no.shape[0]
    mu, a = no[:, :3], no[:, 3:].permute(0, 2, 3, 1)
    U = torch.zeros(a.shape[:3] + (3, 3), dtype=torch.float64)
    for n, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        U[..., i, j] = a[..., n]
    est = None if est_raw is None else (torch.nn.functional.softplus(est_raw.double().reshape(-1) - 4.0) + 1e-3).expand(B).view(B, 1, 1, 1)
    if style.startswith("gauss"):
        var = ((npar.double().view(B, 1, 1, 1).clamp(min=1e-3) if mode == "known" else est) ** 2).expand_as(mu)
    else:
        var = mu.clamp(min=1e-3) * (1.0 / npar.double().view(B, 1, 1, 1) if mode == "known" else est)
    return U @ U.transpose(-1, -2), torch.diag_embed(var.permute(0, 2, 3, 1))


@pytest.mark.parametrize("style,mode", [(s, m) for s in ("gauss25", "poisson30") for m in ("known", "const", "var")])
def test_mirror_covariance_is_the_information_form(style, mode):
    no, y, npar, est = op_inputs(style, mode, 3, H=8, W=8)
    m = posterior_ref(no, y, npar, style, mode, est)
    sx, sn = _sx_sn(no, style, mode, npar, est)
    eye = torch.eye(3, dtype=torch.float64) * EPS
    want = torch.linalg.inv(torch.linalg.inv(sx + eye) + torch.linalg.inv(sn + eye))
    got = full_matrix(m["cov"])
    err, scale = float((got - want).abs().max()), float(want.abs().max())
    print("cov vs information form: max abs err %.3e, largest entry %.3e" % (err, scale))
    assert err <= 1e-9 * scale
    assert torch.equal(m["std"], m["cov"][:, [0, 3, 5]].clamp(min=0).sqrt())
    assert float(torch.linalg.eigvalsh(got).min()) > 0


@pytest.mark.parametrize("style,mode,C", GP_CASES)
def test_mirror_mean_is_the_references_posterior_mean(style, mode, C):
    no, y, npar, est = op_inputs(style, mode, C, H=8, W=8)
    B = no.shape[0]
    m = posterior_ref(no, y, npar, style, mode, est)
    e4 = None if est is None else est.double().reshape(-1, 1, 1, 1)
    ref = R.ssdn_head(no.double(), y.double(), npar.double().view(B, 1, 1, 1), style, mode, e4)["out"]
    err, scale = float((m["mean"] - ref).abs().max()), float(ref.abs().max())
    print("mean vs restate.ssdn_head: max abs err %.3e of %.3e" % (err, scale))
    assert err <= 1e-6 * scale           # (the reference's third eps: (Sx'^-1 + Sn'^-1 + eps I)^-1)


@pytest.mark.parametrize("style,mode", [(s, m) for s in ("gauss25", "poisson30") for m in ("known", "const", "var")])
def test_diagonal_model_is_the_full_model_with_a_diagonal_u(style, mode):
    no6, y, npar, est = op_inputs(style, mode, 3, diag=1, H=8, W=8)
    d = posterior_ref(no6, y, npar, style, mode, est, diag=1)
    f = posterior_ref(scatter9(no6), y, npar, style, mode, est, diag=0)
    assert torch.equal(d["cov"][:, [1, 2, 4]], torch.zeros_like(d["cov"][:, [1, 2, 4]])) and float(f["cov"][:, [1, 2, 4]].abs().max()) == 0.0
    # the eps placement: the diagonal head's rD = 1 / (ix + in + eps) against the full head's 1 / (ix + in): rD_d = rD_f / (1 + eps rD_f)
    dd, ff = d["cov"][:, [0, 3, 5]], f["cov"][:, [0, 3, 5]]
    assert bool(((dd - ff).abs() <= 1.001 * EPS * ff * ff + 1e-18).all()), float((dd - ff).abs().max())
    assert bool(((d["mean"] - f["mean"]).abs() <= 1.001 * EPS * ff * (no6[:, :3].double().abs() + y.double().abs()) + 1e-12).all())


@pytest.mark.parametrize("C,mode,alpha", [(C, mode, a) for C in (1, 3) for mode in ("known", "const", "var") for a in (0.05, 0.5)])
def test_impulse_mixture_mean_is_the_heads_posterior_mean(C, mode, alpha):
    no, y, npar, raw = impulse_inputs(C, mode, alpha)
    est = None if raw is None else (raw.mean(dim=(1, 2, 3)) if mode == "var" else raw)
    m = posterior_ref(no, y, npar, "impulse", mode, est)
    h = impulse_head(no, y, npar, mode, est)
    w = m["w"][:, None]
    mix = w * y.double() + (1 - w) * no[:, :C].double()
    assert float((mix - h["pme"]).abs().max()) <= 1e-12 and float((m["mean"] - h["pme"]).abs().max()) <= 1e-12
    # the mixture's covariance, written out: w (y - m)(y - m)^T + (1 - w) (Sigma_x + (mu - m)(mu - m)^T)
    dy, dm = (y.double() - mix).permute(0, 2, 3, 1), (no[:, :C].double() - mix).permute(0, 2, 3, 1)
    wf = m["w"][..., None, None]
    want = wf * dy[..., :, None] * dy[..., None, :] + (1 - wf) * (full_matrix(m["prior_cov"]) + dm[..., :, None] * dm[..., None, :])
    got = full_matrix(m["cov"])
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


# ---- 3. calibration: data drawn from the model --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("style,kind", [(s, k) for s in ("gauss25", "poisson30") for k in ("full3", "diag3", "mono")])
def test_posterior_is_calibrated_on_data_from_its_own_model(style, kind):
    """net_out is the true prior (|diagonal entries of U| in [0.03, 0.12]: with entries near 0 the eps floor makes Sigma_post wider than
    the true error and the statistic drops); x ~ N(mu, U U^T), y = x + the head's own noise (poisson: N(0, max(mu, 1e-3) / lambda)).
    z = L^-1 (x - pme) is then standard normal: mean z^T z = C within 4 standard errors sqrt(2 C / N)."""
    B, H = 4, 32
    C = 1 if kind == "mono" else 3
    g = torch.Generator().manual_seed(20 + len(style) + 3 * len(kind))
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)          # noqa: E731
    mu = 0.2 + 0.6 * u(B, C, H, H)
    dsign = torch.where(u(B, C, H, H) < 0.5, -1.0, 1.0)
    dmag = (0.03 + 0.09 * u(B, C, H, H)) * dsign
    z = torch.randn(B, C, H, H, generator=g, dtype=torch.float64)
    if kind == "mono":
        A = dmag
        x = mu + A * z
    elif kind == "diag3":
        A = dmag
        x = mu + A * z
    else:
        off = -0.12 + 0.24 * u(B, 3, H, H)
        A = torch.stack([dmag[:, 0], off[:, 0], off[:, 1], dmag[:, 1], off[:, 2], dmag[:, 2]], 1)
        x = torch.stack([mu[:, 0] + A[:, 0] * z[:, 0] + A[:, 1] * z[:, 1] + A[:, 2] * z[:, 2],
                         mu[:, 1] + A[:, 3] * z[:, 1] + A[:, 4] * z[:, 2], mu[:, 2] + A[:, 5] * z[:, 2]], 1)
    npar = torch.full((B,), NPAR[style], dtype=torch.float64)
    var = torch.full_like(mu, NPAR[style] ** 2) if style == "gauss25" else mu.clamp(min=1e-3) / NPAR[style]
    y = x + var.sqrt() * torch.randn(B, C, H, H, generator=g, dtype=torch.float64)
    m = posterior_ref(torch.cat([mu, A], 1), y, npar, style, "known", None, diag=int(kind == "diag3"))
    Lc = torch.linalg.cholesky(full_matrix(m["cov"]))
    r = (x - m["mean"]).permute(0, 2, 3, 1)[..., None]
    zz = torch.linalg.solve_triangular(Lc, r, upper=False)[..., 0]
    N = B * H * H
    stat, se = float((zz * zz).sum(-1).mean()), math.sqrt(2.0 * C / N)
    print("%s %s: mean z^T z = %.4f, expected %d +- %.4f" % (style, kind, stat, C, se))
    assert abs(stat - C) <= 4 * se


# ---- 4. the interface ---------------------------------------------------------------------------------------------------------------------------
def test_denoiser_posterior_refuses_mse_pipelines_and_cpu_devices():
    cfg = ssdn.cfg.base()
    cfg[ConfigValue.ALGORITHM] = NoiseAlgorithm.NOISE_TO_CLEAN
    cfg[ConfigValue.NOISE_STYLE] = "gauss25"
    d = Denoiser(ssdn.cfg.infer(cfg, model_only=True), device="cpu")
    with pytest.raises(NotImplementedError, match="SSDN pipeline only"):
        d.posterior(torch.zeros(1, 3, 32, 32))
    d = Denoiser(diag_cfg("gauss25", "const", diag=False), device="cpu")
    with pytest.raises(L.SsdnHipError, match="no CPU fallback"):
        d.posterior(torch.zeros(1, 3, 32, 32), samples=2)
    assert d._last_engine is None and d._last_train_engine is None


def test_cli_eval_posterior_flag():
    from ssdn.cli.cli import build_parser
    parser, _ = build_parser()
    args = vars(parser.parse_args(["eval", "-m", "x.wt", "-d", "imgs", "--posterior", "2"]))
    assert args["posterior"] == 2
    assert vars(parser.parse_args(["eval", "-m", "x.wt", "-d", "imgs"]))["posterior"] is None
    assert vars(parser.parse_args(["eval", "-m", "x.wt", "-d", "imgs", "--posterior", "0"]))["posterior"] == 0
    with pytest.raises(SystemExit):
        parser.parse_args(["eval", "-m", "x.wt", "-d", "imgs", "--posterior", "-1"])


def test_enums_and_planned_lists_know_nothing_of_the_op():
    from ssdn.params import PipelineOutput
    assert not any("cov" in o.name.lower() or "posterior" in o.name.lower() for o in PipelineOutput)
    src = open(os.path.join(ROOT, "selfsupervised-denoising_amd", "ssdn", "hip", "graph.py")).read()
    assert "head_posterior" not in src
