"""CPU: DIAGONAL_COVARIANCE on the SSDN pipeline.  The Denoiser builds with 2*C outputs in the reference's key
layout; the diagonal head's per-channel closed forms, restated in float64 torch (`diag_head64`), agree with autograd of the oracle's full
head (oracle/restate.py::ssdn_head) applied to the 6-channel output scattered into the 9 triangular channels (a_0, 0, 0, a_1, 0, a_2);
the planner lowers a 6-output network; `ssdn train start --diagonal` builds the model.  The GPU tests (tests/test_hip_diag_cov.py) reuse
`diag_inputs`, `diag_head64`, `scatter9` and `oracle_diag`."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import restate as R
import ssdn
from ssdn.denoiser import Denoiser
from ssdn.params import ConfigValue, NoiseAlgorithm, NoiseValue

CASES = [(style, mode) for style in ("gauss25", "poisson30") for mode in ("known", "const", "var")]
NPAR = {"gauss25": 25 / 255.0, "poisson30": 30.0}
DIAG_CH = (3, 6, 8)            # where a_0, a_1, a_2 sit among the full head's 9 channels (upper triangle of U, row-major)


def diag_cfg(style="gauss25", mode="known", ch=3, diag=True):
    cfg = ssdn.cfg.base()
    cfg[ConfigValue.ALGORITHM] = NoiseAlgorithm.SELFSUPERVISED_DENOISING
    cfg[ConfigValue.NOISE_STYLE] = style
    cfg[ConfigValue.NOISE_VALUE] = NoiseValue(mode)
    cfg[ConfigValue.IMAGE_CHANNELS] = ch
    cfg[ConfigValue.DIAGONAL_COVARIANCE] = diag
    return ssdn.cfg.infer(cfg, model_only=True)


def diag_inputs(style, mode, B=2, H=8, seed=0):
    """net_out [B,6,H,W] (means in (0.05, 0.95), a_c in (-0.4, 0.6) with a few pixels at a_c = 0 -- one with all three -- and a poisson
    mean below the 1e-3 clamp), noisy, noise parameter [B], raw estimate (var: map [B,1,H,W]; const: [1]), all float32"""
    net_out = R.hash_tensor((B, 6, H, H), 141 + seed, -0.4, 0.6)
    net_out[:, :3] = R.hash_tensor((B, 3, H, H), 142 + seed, 0.05, 0.95)
    net_out[0, 3, 0, 0] = 0.0
    net_out[1, 4:6, 2, 3] = 0.0
    net_out[0, 3:6, 1, 2] = 0.0
    net_out[1, 5, 4, 4] = -0.35
    net_out[0, 1, 3, 5] = 5e-4
    noisy = R.hash_tensor((B, 3, H, H), 143 + seed, 0.0, 1.0)
    npar = torch.full((B,), NPAR[style])
    raw = None
    if mode == "var":
        raw = R.hash_tensor((B, 1, H, H), 144 + seed, 1.0, 3.0)
    elif mode == "const":
        raw = torch.full((1,), 1.7)
    return net_out, noisy, npar, raw


def scatter9(net_out6):
    """the diagonal model as the full head: triangular entries (a_0, 0, 0, a_1, 0, a_2)"""
    B, _, H, W = net_out6.shape
    o = torch.zeros((B, 9, H, W), dtype=net_out6.dtype)
    o[:, :3] = net_out6[:, :3]
    for c, k in enumerate(DIAG_CH):
        o[:, k] = net_out6[:, 3 + c]
    return o


def diag_head64(net_out, noisy, npar, style, mode, est_raw, w=None, g_pme=None, g_mu=None):
    """The kernels' per-pixel formulas (k_head<true>, k_head_vjp<GY, true>) in float64.  est_raw: [1] (const) or [B] (var) pre-softplus.
    -> dict: loss [B], mu, pme [B,3,H,W], model_std [B,H,W], noise_std ([B] gauss, [B,H,W] poisson), and for the upstream gradients
    w = dL/dLOSS [B], g_pme, g_mu: g_net_out = dL/dnet_out [B,6,H,W], g_est = dL/dest_raw ([1] const, [B] var, None known),
    g_noisy = the head's direct dL/dnoisy [B,3,H,W]"""
    d64 = lambda t: None if t is None else t.double()    # noqa: E731
    no, y = d64(net_out), d64(noisy)
    w, gp, gm = d64(w), d64(g_pme), d64(g_mu)
    B, _, H, W = no.shape
    HW = H * W
    sc = (w if w is not None else torch.zeros(B, dtype=torch.float64)).view(B, 1, 1, 1) / HW
    mu, av = no[:, :3], no[:, 3:]
    if mode != "known":
        raw = d64(est_raw).reshape(-1)
        raw = raw.expand(B) if raw.numel() == 1 else raw
        est, dest_draw = (F.softplus(raw - 4.0) + 1e-3).view(B, 1, 1, 1), torch.sigmoid(raw - 4.0).view(B, 1, 1, 1)
    npar = d64(npar).view(B, 1, 1, 1)
    if style.startswith("gauss"):
        sig = (npar.clamp(min=1e-3) if mode == "known" else est).expand(B, 3, H, W)
        dsig_dmu, dsig_dest = torch.zeros_like(mu), torch.ones_like(mu)
    else:
        m = mu.clamp(min=1e-3)
        f = 1.0 / npar if mode == "known" else est
        sig = (m * f).sqrt()
        dsig_dmu = torch.where(mu > 1e-3, 0.5 * f / sig, torch.zeros_like(mu))
        dsig_dest = 0.5 * m / sig
    reg = 0.1 if mode != "known" else 0.0
    e = 1e-6
    sx, sn = av ** 2, sig ** 2
    sy = sx + sn
    d = y - mu
    q = d / sy
    prod = sy.prod(1)
    l = 0.5 * torch.log(prod.clamp(min=0)) + 0.5 * (d * q).sum(1)
    if mode != "known":
        l = l - reg * sig.mean(1)
    ix, iN = 1 / (sx + e), 1 / (sn + e)
    rD = 1 / (ix + iN + e)
    u, v = ix * rD, iN * rD
    out = dict(loss=l.reshape(B, -1).mean(1), mu=mu, pme=mu * u + y * v, model_std=(sx.prod(1)).clamp(min=0) ** (1 / 6))
    out["noise_std"] = sig[:, 0, 0, 0] if style.startswith("gauss") else sn.prod(1) ** (1 / 6)
    # the vector-Jacobian product
    hd = 0.5 * (prod > 0).double()[:, None]
    dsy = (hd / sy - 0.5 * q * q) * sc
    dsx, dn, gmu = dsy.clone(), dsy.clone(), -q * sc
    gy = q * sc
    if gp is not None:
        gmu = gmu + gp * u
        dsx = dsx + gp * (d * v - mu * e * rD) * ix * u            # (pme - mu) ix^2 / D
        dn = dn - gp * (d * u + y * e * rD) * iN * v               # (pme - y) in^2 / D
        gy = gy + gp * v
    ds = 2 * sig * dn - reg / 3.0 * sc
    gmu = gmu + ds * dsig_dmu + (gm if gm is not None else 0)
    out["g_net_out"] = torch.cat([gmu, 2 * av * dsx], 1)
    out["g_noisy"] = gy
    out["g_est"] = None
    if mode != "known":
        gest = (ds * dsig_dest).sum(dim=(1, 2, 3)) * dest_draw.view(B)
        out["g_est"] = gest.sum().view(1) if mode == "const" else gest
    return out


def oracle_diag(net_out, noisy, npar, style, mode, raw, w=None, g_pme=None, g_mu=None):
    """float64 autograd of R.ssdn_head on the scattered output -> (outputs dict, dL/dnet_out [B,6,H,W], dL/d(raw: scalar or var map),
    dL/dnoisy)"""
    B = net_out.shape[0]
    no = net_out.double().requires_grad_(True)
    y = noisy.double().requires_grad_(True)
    raw64 = est64 = None
    if raw is not None:
        raw64 = raw.double().reshape((B, 1) + tuple(raw.shape[2:]) if mode == "var" else (1, 1, 1, 1)).requires_grad_(True)
        est64 = raw64.mean(dim=(2, 3), keepdim=True) if mode == "var" else raw64
    o = R.ssdn_head(scatter9(no), y, npar.double().view(B, 1, 1, 1), style, mode, est64)
    L = 0
    if w is not None:
        L = L + (o["loss"].view(B) * w.double()).sum()
    if g_pme is not None:
        L = L + (o["out"] * g_pme.double()).sum()
    if g_mu is not None:
        L = L + (o["out_mu"] * g_mu.double()).sum()
    gs = torch.autograd.grad(L, [no, y] + ([raw64] if raw64 is not None else []), allow_unused=True)
    gs = [torch.zeros_like(t) if g is None else g for g, t in zip(gs, [no, y] + ([raw64] if raw64 is not None else []))]
    o = {k: v.detach() for k, v in o.items()}
    return o, gs[0], (gs[2] if raw64 is not None else None), gs[1]


def _close(a, b, rel, what=""):
    err = float((a - b).abs().max())
    scale = float(b.abs().max())
    assert err <= rel * scale + 1e-300, "%s: max abs err %.3e vs scale %.3e" % (what, err, scale)


# ---- the model ----------------------------------------------------------------------------------------------------------------------------
def test_diag_denoiser_state_dict_layout(golden_dir):
    d = Denoiser(diag_cfg(), device="cpu")
    sd = d.state_dict()
    want = json.load(open(os.path.join(golden_dir, "g_ckpt_contract.json")))["ssdn_known"]
    assert list(sd.keys()) == want["keys"]
    out_layer = ("output_block.4.", "output_conv.")
    for k, shp in want["shapes"].items():
        if any(s in k for s in out_layer):
            assert list(sd[k].shape) == ([6, 96, 1, 1] if k.endswith("weight") else [6]), k
        else:
            assert list(sd[k].shape) == shp, k
    assert sd["_models.denoiser_model.output_conv.weight"].data_ptr() == sd["_models.denoiser_model.output_block.4.weight"].data_ptr()
    assert d.config_name() == want["config_name"] + "-diag"
    # from_state_dict / load_state_dict keep the layout and the values
    for k, v in sd.items():
        if k != "cfg":
            v.copy_(R.hash_tensor(tuple(v.shape), 7, -1, 1))
    back = Denoiser.from_state_dict(sd)
    sd2 = back.state_dict()
    assert list(sd2.keys()) == list(sd.keys()) and sd2["cfg"][ConfigValue.DIAGONAL_COVARIANCE] is True
    for k in sd:
        if k != "cfg":
            assert torch.equal(sd2[k].cpu(), sd[k]), k


def test_diag_mono_is_the_mono_model():
    """C = 1: the reference builds 2 outputs with or without the flag; only the run name differs"""
    a, b = Denoiser(diag_cfg(ch=1, diag=True), device="cpu"), Denoiser(diag_cfg(ch=1, diag=False), device="cpu")
    sa, sb = a.state_dict(params_only=True), b.state_dict(params_only=True)
    assert list(sa) == list(sb) and all(sa[k].shape == sb[k].shape for k in sa)
    assert a.flat.numel() == b.flat.numel()
    assert a.config_name() == b.config_name() + "-diag"


def test_diag_ignored_by_mse_pipelines():
    cfg = ssdn.cfg.base()
    cfg[ConfigValue.ALGORITHM] = NoiseAlgorithm.NOISE_TO_CLEAN
    cfg[ConfigValue.NOISE_STYLE] = "gauss25"
    cfg[ConfigValue.DIAGONAL_COVARIANCE] = True
    d = Denoiser(ssdn.cfg.infer(cfg, model_only=True), device="cpu")
    assert d.state_dict()["_models.denoiser_model.output_block.4.bias"].shape == (3,)


# ---- the head's closed forms --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("style,mode", CASES)
def test_diag_forward_vs_scattered_full_head(style, mode):
    net_out, noisy, npar, raw = diag_inputs(style, mode)
    B = net_out.shape[0]
    est_raw = raw.double().mean(dim=(1, 2, 3)) if mode == "var" else raw
    m = diag_head64(net_out, noisy, npar, style, mode, est_raw, w=torch.full((B,), 1.0 / B))
    o, g, graw, _ = oracle_diag(net_out, noisy, npar, style, mode, raw, w=torch.full((B,), 1.0 / B))
    _close(m["loss"], o["loss"].view(B), 1e-12, "loss")
    _close(m["mu"], o["out_mu"], 0, "mu")
    _close(m["pme"], o["out"], 1e-12, "pme")
    _close(m["model_std"], o["model_std"], 1e-12, "model_std")
    ons = o["noise_std"].reshape(-1)
    if style.startswith("gauss"):                                   # (one value per sample; for a learnt constant one for the batch)
        ons = ons.expand(B) if ons.numel() == 1 else o["noise_std"].reshape(B, -1)[:, 0]
    _close(m["noise_std"].reshape(-1), ons, 1e-12, "noise_std")
    assert float(m["model_std"][0, 1, 2]) == 0.0                  # all three a_c = 0: a singular Sigma_x
    _close(m["g_net_out"], g, 1e-10, "dL/dnet_out of mean(LOSS)")
    H = net_out.shape[2]
    if mode == "const":
        _close(m["g_est"], graw.reshape(1), 1e-10, "g_est")
    if mode == "var":
        _close(m["g_est"].view(B, 1, 1, 1).expand_as(graw) / (H * H), graw, 1e-10, "g_sigma_out")


@pytest.mark.parametrize("style,mode", CASES)
@pytest.mark.parametrize("terms", ["all", "loss", "pme", "mu"])
def test_diag_vjp_and_noisy_grad_vs_autograd(style, mode, terms):
    net_out, noisy, npar, raw = diag_inputs(style, mode, seed=1)
    B, H = net_out.shape[0], net_out.shape[2]
    g = torch.Generator().manual_seed(11)
    f = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    w = f(B) if terms in ("all", "loss") else None
    gp = f(B, 3, H, H) if terms in ("all", "pme") else None
    gm = f(B, 3, H, H) if terms in ("all", "mu") else None
    est_raw = raw.double().mean(dim=(1, 2, 3)) if mode == "var" else raw
    m = diag_head64(net_out, noisy, npar, style, mode, est_raw, w, gp, gm)
    _, og, oraw, ody = oracle_diag(net_out, noisy, npar, style, mode, raw, w, gp, gm)
    _close(m["g_net_out"], og, 1e-10, "dL/dnet_out")
    if terms != "mu":
        _close(m["g_noisy"], ody, 1e-10, "dL/dnoisy")
    else:
        assert float(m["g_noisy"].abs().max()) == 0.0 and float(ody.abs().max()) == 0.0
    if mode == "const":
        _close(m["g_est"], oraw.reshape(1), 1e-10, "g_est")
    if mode == "var":
        _close(m["g_est"].view(B, 1, 1, 1).expand_as(oraw) / (H * H), oraw, 1e-10, "g_sigma_out")


# ---- the lowering of a 6-output network ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev_cus", [None, 8])
def test_forward_backward_lowering_six_outputs(dev_cus):
    from test_lowering_cpu import _check_lowering
    torch.set_default_dtype(torch.float64)
    try:
        _check_lowering(3, 6, True, 2, 32, 32, dev_cus)
    finally:
        torch.set_default_dtype(torch.float32)


# ---- the command line ---------------------------------------------------------------------------------------------------------------------
def test_cli_train_start_diagonal_builds_the_model(tmp_path, monkeypatch):
    from ssdn.cli.cli import build_parser
    from ssdn.train import DenoiserTrainer
    built = {}

    def fake_train(self):            # (the run itself needs a GPU: stop where the model has been built)
        self.new_target()
        built["trainer"] = self

    monkeypatch.setattr(DenoiserTrainer, "train", fake_train)
    parser, cmds = build_parser()
    h5 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g_libhdf5_dataset.h5")
    args = vars(parser.parse_args(["train", "start", "-a", "ssdn", "-n", "gauss25", "--noise_value", "known", "--diagonal", "-t", h5,
                                   "-i", "1000", "--runs_dir", str(tmp_path)]))
    assert args["diagonal"] is True
    args["PARSER"] = parser
    cmds["train"].execute(args)
    tr = built["trainer"]
    assert tr.cfg[ConfigValue.DIAGONAL_COVARIANCE] is True
    d = tr.denoiser
    assert d.config_name().endswith("-diag")
    assert d.state_dict()["_models.denoiser_model.output_block.4.weight"].shape == (6, 96, 1, 1)
