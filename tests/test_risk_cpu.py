"""CPU: the reference-free risk estimate (ssdn.utils.calculate_risk / risk_values, SSDN_OP_RISK, `--risk`, `--noisy_validation`): the
float64 specification by hand and against numpy.linalg, the two identities it rests on with a toy blind function, the C ABI of the op and
its argument rules (raised before any device call, so they show without a GPU), and the opt-in switches of the library, the command
line and the trainer."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import risk_ref as R
from ssdn.hip import lib as L
from ssdn.utils import calculate_risk, risk_values
from ssdn.utils import data as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUES = ["mse_mu_est", "mse_out_est", "psnr_mu_est", "psnr_out_est", "mse_mu_se", "mse_out_se", "nll", "weight", "clipped", "degenerate"]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _definition(inp, ext=None, margin=0, maps=False):
    """calculate_risk fed with what the numpy model builds from an op's inputs"""
    Cn = inp["noisy"].shape[1]
    mu, cov, n, v = R.definition_inputs(inp["net_out"], inp["noisy"], inp["noise_param"], inp["est_raw"], Cn, inp["style"], inp["mode"], inp["diag"])
    return calculate_risk(_t(inp["noisy"]), _t(mu), _t(cov), _t(inp["pme"]), _t(n), _t(v), ext=ext, margin=margin, maps=maps)


# ---- 1. the specification -------------------------------------------------------------------------------------------------------------------
def test_one_channel_by_hand():
    """mu 0.5, s 0.01, n 0.01, y 0.7, out 0.6: W = 1/2, q_mu = 0.04 - 0.01, q_out = 0.01 + 0"""
    one = lambda v: torch.full((1, 1, 1, 1), v, dtype=torch.float64)      # noqa: E731
    res = calculate_risk(one(0.7), one(0.5), one(0.01), one(0.6), one(0.01), one(0.01), maps=True)
    assert set(res) == set(VALUES) | {"stats", "q_mu", "q_out"} and D.RISK_VALUES == tuple(VALUES) and D.RISK_NSTATS == 12
    s = res["stats"]
    assert s.dtype == torch.float64 and tuple(s.shape) == (1, 12)
    want = [1, 0, 0.2 ** 2 / 0.02, math.log(0.02), 0.2 ** 2, 0.1 ** 2, 0.01, 0.0, 0.03 ** 2, 0.01 ** 2, 0.5, 0]
    np.testing.assert_allclose(s[0].numpy(), want, rtol=1e-12, atol=1e-17)
    assert abs(float(res["q_mu"]) - 0.03) <= 1e-15 and abs(float(res["q_out"]) - 0.01) <= 1e-15 and res["q_mu"].shape == (1, 1, 1)
    # one pixel: N < 2, every ratio is NaN; the share of degenerate pixels is defined
    assert all(math.isnan(float(res[k])) for k in VALUES[:-1]) and float(res["degenerate"]) == 0.0
    # two such pixels: the values
    two = calculate_risk(*(t.expand(1, 1, 1, 2) for t in (one(0.7), one(0.5), one(0.01), one(0.6), one(0.01), one(0.01))))
    assert abs(float(two["mse_mu_est"]) - 0.03) <= 1e-15 and abs(float(two["mse_out_est"]) - 0.01) <= 1e-15
    assert abs(float(two["psnr_out_est"]) - 20.0) <= 1e-12 and abs(float(two["psnr_mu_est"]) + 10 * math.log10(0.03)) <= 1e-12
    assert float(two["mse_mu_se"]) <= 1e-12 and float(two["weight"]) == 0.5 and float(two["clipped"]) == 0.0
    assert abs(float(two["nll"]) - (0.5 * (2.0 + math.log(0.02)) + 0.5 * math.log(2 * math.pi))) <= 1e-14


@pytest.mark.parametrize("Cn,style,mode,diag", [(1, "gauss", "known", False), (3, "gauss", "known", False), (3, "poisson", "known", False),
                                                (3, "gauss", "const", True), (3, "poisson", "var", False), (1, "poisson", "const", False)])
def test_against_numpy_linalg(Cn, style, mode, diag):
    inp = R.make_inputs(2, Cn, 9, 13, style, mode, diag, seed=Cn)
    res = _definition(inp, maps=True)
    want, _, px = R.risk_model(inp["net_out"], inp["noisy"], inp["pme"], inp["noise_param"], inp["est_raw"], inp["style"], inp["mode"], inp["diag"])
    s = res["stats"].numpy()
    for k in R.COUNTS:
        assert (s[:, k] == want[:, k]).all(), (k, s[:, k], want[:, k])
    assert (s[:, 0] == 9 * 13).all() and (s[:, 1] == 0).all()
    for k in R.FLOAT_SUMS:
        np.testing.assert_allclose(s[:, k], want[:, k], rtol=1e-9, atol=0, err_msg="statistic %d" % k)
    np.testing.assert_allclose(res["q_mu"].numpy(), px["q_mu"], rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(res["q_out"].numpy(), px["q_out"], rtol=1e-9, atol=1e-15)
    # the reported values from the raw statistics
    n, nc = s[:, 0], s[:, 0] * Cn
    val = risk_values(res["stats"], Cn)
    assert list(val) == VALUES and all(torch.equal(val[k], res[k]) for k in VALUES if not torch.isnan(val[k]).any())
    np.testing.assert_allclose(res["mse_mu_est"].numpy(), (s[:, 4] - s[:, 6]) / nc, rtol=1e-15)
    np.testing.assert_allclose(res["mse_out_est"].numpy(), (s[:, 5] + s[:, 7]) / nc, rtol=1e-15)
    with np.errstate(invalid="ignore"):                  # (the builder's pme is arbitrary: an estimate may be <= 0, its PSNR NaN on both sides)
        np.testing.assert_allclose(res["psnr_out_est"].numpy(), -10 * np.log10((s[:, 5] + s[:, 7]) / nc), rtol=1e-14)
        np.testing.assert_allclose(res["psnr_mu_est"].numpy(), -10 * np.log10((s[:, 4] - s[:, 6]) / nc), rtol=1e-14)
    for name, sq, k in (("mse_mu_se", s[:, 4] - s[:, 6], 8), ("mse_out_se", s[:, 5] + s[:, 7], 9)):
        np.testing.assert_allclose(res[name].numpy(), np.sqrt((s[:, k] - sq ** 2 / n) / (n * (n - 1))) / Cn, rtol=1e-12)
    np.testing.assert_allclose(res["nll"].numpy(), 0.5 * (s[:, 2] + s[:, 3]) / nc + 0.5 * math.log(2 * math.pi), rtol=1e-15)
    np.testing.assert_allclose(res["weight"].numpy(), s[:, 10] / nc, rtol=1e-15)
    assert ((0 < res["weight"].numpy()) & (res["weight"].numpy() < 1)).all()


def test_degenerate_and_clipped_pixels():
    inp = R.make_inputs(2, 3, 6, 7, seed=7)
    noisy, (mu, cov, n, v) = inp["noisy"].copy(), [a.copy() for a in R.definition_inputs(inp["net_out"], inp["noisy"], inp["noise_param"], inp["est_raw"], 3, 0, 0, 0)]
    out = inp["pme"].copy()
    base = calculate_risk(_t(noisy), _t(mu), _t(cov), _t(out), _t(n), _t(v), maps=True)
    mu[0, 1, 3, 3] = np.nan
    out[0, 2, 0, 0] = np.inf
    cov[0, :, 1, 2], n[0, :, 1, 2] = 0.0, 0.0                                      # T = 0: p0 = 0
    cov[0, :, 4, 5], n[0, :, 4, 5] = [1.0, 1.0, 0.0, 1.0, 0.0, 1.0], 0.0           # the exact singular [[1,1,0],[1,1,0],[0,0,1]]: p1 = 0
    n[0, 0, 5, 6] = -1.0                                                           # a negative pivot
    v[0, 1, 2, 2] = np.nan
    noisy[0, 0, 0, 1], noisy[0, 2, 0, 1], noisy[0, 1, 5, 0] = 0.0, 1.0, -0.25      # three clipped samples in two valid pixels
    noisy[0, 0, 3, 3] = 1.5                                                        # ... and one in a degenerate pixel: not counted
    bad = [(3, 3), (0, 0), (1, 2), (4, 5), (5, 6), (2, 2)]
    res = calculate_risk(_t(noisy), _t(mu), _t(cov), _t(out), _t(n), _t(v), maps=True)
    keep = torch.ones(6, 7, dtype=torch.bool)
    for i, j in bad:
        keep[i, j] = False
    alone = calculate_risk(*(_t(a)[:1, :, keep][:, :, None] for a in (noisy, mu, cov, out, n, v)))
    s = res["stats"]
    nclip = int(((noisy[0] <= 0) | (noisy[0] >= 1))[:, keep.numpy()].sum())              # the planted three and what the builder's noise gave
    assert nclip >= 3 and nclip == int(((inp["noisy"][0] <= 0) | (inp["noisy"][0] >= 1))[:, keep.numpy()].sum()) + 3
    assert s[0, 0] == 36 and s[0, 1] == 6 and float(res["degenerate"][0]) == 6 / 42 and s[0, 11] == nclip and float(res["clipped"][0]) == nclip / 108
    assert torch.equal(s[0, [0, 11]], alone["stats"][0, [0, 11]]) and torch.isfinite(s).all()
    assert torch.allclose(s[0, 2:11], alone["stats"][0, 2:11], rtol=1e-12, atol=0)
    assert torch.equal(torch.isnan(res["q_mu"][0]), ~keep) and torch.equal(torch.isnan(res["q_out"][0]), ~keep)
    assert torch.equal(s[1], base["stats"][1]) and torch.equal(res["q_out"][1], base["q_out"][1])
    # no valid pixel at all: the ratios are NaN, the counts stay
    none = calculate_risk(*(_t(a)[:1, :, 1:2, 2:3] for a in (noisy, mu, cov, out, n, v)))
    assert none["stats"][0].tolist() == [0, 1] + [0] * 10
    assert all(math.isnan(float(none[k])) for k in VALUES[:-1]) and float(none["degenerate"]) == 1.0


def test_extent_and_margin():
    inp = R.make_inputs(2, 3, 10, 12, seed=2)
    full = _definition(inp, maps=True)
    ext = [[10, 12], [7, 5]]
    for margin in (0, 1, 2):
        res = _definition(inp, ext=torch.tensor(ext), margin=margin, maps=True)
        for b, (e1, e2) in enumerate(ext):
            crop = lambda a: a[b:b + 1, :, margin:e1 - margin, margin:e2 - margin]      # noqa: E731
            one = dict(inp, **{k: np.ascontiguousarray(crop(inp[k])) for k in ("net_out", "noisy", "pme")},
                       noise_param=inp["noise_param"][b:b + 1], est_raw=inp["est_raw"][b:b + 1])
            alone = _definition(one)
            assert res["stats"][b, 0] == (e1 - 2 * margin) * (e2 - 2 * margin) == alone["stats"][0, 0]
            assert torch.allclose(res["stats"][b], alone["stats"][0], rtol=1e-12, atol=0)
            inside = torch.zeros(10, 12, dtype=torch.bool)
            inside[margin:e1 - margin, margin:e2 - margin] = True
            assert torch.equal(~torch.isnan(res["q_out"][b]), inside)
            assert torch.equal(res["q_out"][b][inside], full["q_out"][b][inside])
    # a margin that leaves nothing (2 margin >= the extent in an axis), and an extent outside the tensor (clamped)
    empty = _definition(inp, ext=torch.tensor(ext), margin=3)
    assert empty["stats"][0, 0] == 4 * 6 and empty["stats"][1].tolist() == [0] * 12 and math.isnan(float(empty["psnr_out_est"][1]))
    assert math.isnan(float(empty["degenerate"][1]))
    big = _definition(inp, ext=torch.tensor([[99, 99], [-3, 5]]))
    assert torch.equal(big["stats"][0], full["stats"][0]) and big["stats"][1].tolist() == [0] * 12
    assert _definition(inp, margin=100)["stats"].abs().sum() == 0
    with pytest.raises(ValueError, match="calculate_risk: margin"):
        _definition(inp, margin=-1)


def test_shapes_are_checked():
    inp = R.make_inputs(1, 3, 4, 5)
    y, o = _t(inp["noisy"]), _t(inp["pme"])
    m, c, n, v = (_t(a) for a in R.definition_inputs(inp["net_out"], inp["noisy"], inp["noise_param"], inp["est_raw"], 3, 0, 0, 0))
    for bad in ((y[:, :2], m[:, :2], c, o[:, :2], n[:, :2], v[:, :2]), (y, m, c[:, :5], o, n, v), (y[0], m[0], c[0], o[0], n[0], v[0]),
                (y, m, c, o[:, :, :3], n, v), (y, m, c, o, n, v[:, :1])):
        with pytest.raises(ValueError, match="calculate_risk"):
            calculate_risk(*bad)


# ---- 2. the identities ----------------------------------------------------------------------------------------------------------------------
IDENTITY_CASES = [(Cn, style, seed) for Cn in (1, 3) for style in ("gauss", "poisson") for seed in (0, 1, 2)]


def _identity(Cn, style, seed):
    """-> per output (mean of q - |. - x|^2, its naive standard error, the same with the sign of the (2W - 1) term flipped)"""
    clean = R.toy_clean(Cn)
    noisy = R.toy_noisy(clean, style, seed)
    mu, S, n, v, out, wcc = R.toy_blind(noisy, style)
    cov = np.stack([S[..., i, j] for i, j in (R.TRI if Cn == 3 else ((0, 0),))])
    res = calculate_risk(*(_t(a)[None] for a in (noisy, mu, cov, out, n, v)), maps=True)
    N = clean.shape[1] * clean.shape[2]
    assert float(res["stats"][0, 0]) == N and float(res["stats"][0, 1]) == 0
    np.testing.assert_allclose(res["stats"][0, 10].item(), wcc.sum(), rtol=1e-9)        # the definition's W is the toy function's
    rows = {}
    for name, est in (("mu", mu), ("out", out)):
        d = res["q_" + name][0].numpy() - ((est - clean) ** 2).sum(0)
        rows[name] = (d.mean(), d.std() / math.sqrt(N))
    flipped = ((out - noisy) ** 2).sum(0) - ((2 * wcc - 1) * v).sum(0) - ((out - clean) ** 2).sum(0)
    rows["flipped"] = (flipped.mean(), flipped.std() / math.sqrt(N))
    return rows


@pytest.mark.parametrize("Cn,style,seed", IDENTITY_CASES)
def test_the_two_identities_with_a_toy_blind_function(Cn, style, seed):
    """E|mu - x|^2 = E[q_mu], E|out - x|^2 = E[q_out] for a prior that is a function of the other pixels only: the mean difference over
    48 x 64 pixels lies within 5 naive standard errors of 0 (the calibration tests' five standard deviations); with the sign of the
    (2 W - 1) term flipped the same bound fails, so the test can fail."""
    rows = _identity(Cn, style, seed)
    for name in ("mu", "out"):
        mean, se = rows[name]
        print("C %d %s seed %d %s: mean %.3e, se %.3e, ratio %.2f" % (Cn, style, seed, name, mean, se, mean / se))
        assert abs(mean) <= 5 * se, (name, mean / se)
    mean, se = rows["flipped"]
    print("flipped: ratio %.2f" % (mean / se))
    assert abs(mean) > 5 * se


# ---- 3. the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_struct_size():
    hdr = open(os.path.join(ROOT, "include", "ssdn_hip.h")).read()
    assert re.search(r"SSDN_OP_RISK\s*=\s*40\b", hdr) and "} ssdn_risk_args;" in hdr
    assert re.search(r"#define SSDN_ABI_VERSION 19\b", hdr) and L.ABI_VERSION == 19
    assert L.OP["risk"] == 40 and L.ARG_TYPES["risk"] is L.RiskArgs
    assert [n for n, _ in L.RiskArgs._fields_] == ["net_out", "noisy", "noise_param", "est_raw", "pme", "ext", "B", "C", "H", "W", "style", "mode",
                                                   "diag", "margin", "stats", "scratch", "scratch_bytes"]
    assert L.load().ssdn_struct_size(40) == C.sizeof(L.RiskArgs) == 104
    blk, ns = (int(re.search(r"#define SSDN_RISK_%s (\d+)" % a, hdr).group(1)) for a in ("BLOCK", "NSTATS"))
    assert (blk, ns) == (L.RISK_BLOCK, L.RISK_NSTATS) == (256, D.RISK_NSTATS)
    assert "#define SSDN_RISK_SCRATCH_BYTES(B, C, H, W)" in hdr
    assert L.risk_scratch_bytes(2, 3, 8, 8) == 96 * 2 and L.risk_scratch_bytes(3, 3, 37, 70) == 96 * 3 * 11 and L.risk_scratch_bytes(1, 1, 16, 16) == 96
    # the kernel file repeats the definition and keeps its products and sums apart
    src = open(os.path.join(ROOT, "selfsupervised-denoising_amd", "csrc", "risk.hip")).read()
    assert "#pragma clang fp contract(off)" in src.split("#include")[0] and "k_risk_final" in src and "Li20" in src
    mk = open(os.path.join(ROOT, "selfsupervised-denoising_amd", "csrc", "Makefile")).read()
    assert re.search(r"check_scratch\.py \$@ k_risk\b", mk) and " risk.hip " in mk


def _refused(**kw):
    """run one op with dummy (never dereferenced) pointers -> the library's error text"""
    f = dict(net_out=0x1000, noisy=0x1000, noise_param=0x1000, est_raw=None, pme=0x1000, ext=None, B=1, C=3, H=16, W=16, style=0, mode=0,
             diag=0, margin=0, stats=0x1000, scratch=0x1000, scratch_bytes=1 << 20)
    f.update(kw)
    a = L.RiskArgs(**f)
    rec = (L.OpRec * 1)()
    rec[0].type, rec[0].lane, rec[0].args = L.OP["risk"], 0, C.cast(C.pointer(a), C.c_void_p)
    lib = L.load()
    assert lib.ssdn_run_ops(rec, 1, None) != 0
    return lib.ssdn_last_error().decode()


@pytest.mark.parametrize("kw,msg", [
    (dict(net_out=None), "net_out, noisy and pme must be given"),
    (dict(noisy=None), "net_out, noisy and pme must be given"),
    (dict(pme=None), "net_out, noisy and pme must be given"),
    (dict(stats=None), "the output stats must be given"),
    (dict(scratch=None), "scratch must be given"),
    (dict(C=2), "C must be 1 or 3"),
    (dict(C=0), "C must be 1 or 3"),
    (dict(C=4), "C must be 1 or 3"),
    (dict(B=0), "B, H and W must be at least 1"),
    (dict(H=0), "B, H and W must be at least 1"),
    (dict(W=-1), "B, H and W must be at least 1"),
    (dict(margin=-1), "margin must be at least 0"),
    (dict(style=2), "style 2 \\(impulse\\) is not supported.*not affine.*not zero-mean"),
    (dict(style=3), "style must be 0 \\(gauss\\) or 1 \\(poisson\\)"),
    (dict(style=-1), "style must be 0 \\(gauss\\) or 1 \\(poisson\\)"),
    (dict(mode=3), "mode must be 0, 1 or 2"),
    (dict(mode=-1), "mode must be 0, 1 or 2"),
    (dict(noise_param=None), "mode known needs noise_param"),
    (dict(mode=1), "modes const / var need est_raw"),
    (dict(mode=2, noise_param=None), "modes const / var need est_raw"),
    (dict(diag=2), "diag must be 0 or 1"),
    (dict(diag=-1), "diag must be 0 or 1"),
    (dict(scratch_bytes=95), "scratch_bytes is below"),
    (dict(H=17, scratch_bytes=96), "scratch_bytes is below"),
    (dict(scratch=0x1004), "scratch must be 8-byte aligned"),
    (dict(B=65536, scratch_bytes=1 << 40), "B must be at most 65535"),
    (dict(H=1 << 16, W=1 << 15, scratch_bytes=1 << 40), "H \\* W at most"),
])
def test_run_ops_refuses_bad_arguments_without_a_gpu(kw, msg):
    err = _refused(**kw)
    assert re.search(r"^op 0 \(type 40\): risk: .*" + msg, err), err


def test_planned_lists_know_nothing_of_the_op():
    for f in (("selfsupervised-denoising_amd", "ssdn", "hip", "graph.py"), ("oracle", "interp.py")):
        assert "risk" not in open(os.path.join(ROOT, *f)).read().lower()


# ---- 4. the switches ------------------------------------------------------------------------------------------------------------------------
def _cpu_denoiser(algorithm="ssdn", style="gauss25", value="known"):
    import ssdn
    from ssdn.denoiser import Denoiser
    from ssdn.params import ConfigValue, NoiseAlgorithm, NoiseValue
    cfg = ssdn.cfg.base()
    cfg[ConfigValue.ALGORITHM] = NoiseAlgorithm(algorithm)
    cfg[ConfigValue.NOISE_STYLE] = style
    if algorithm == "ssdn":
        cfg[ConfigValue.NOISE_VALUE] = NoiseValue(value)
    return Denoiser(ssdn.cfg.infer(cfg, model_only=True), device="cpu")


def _save(d, path):
    torch.save({k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in d.state_dict().items()}, path)


def test_parsers_and_help_texts():
    from ssdn.cli.cli import build_parser
    parser, _ = build_parser()
    den = ["denoise", "-m", "x.wt", "-i", "in", "-o", "out"]
    off, on = vars(parser.parse_args(den)), vars(parser.parse_args(den + ["--risk", "--risk_margin", "4"]))
    assert off["risk"] is False and off["risk_margin"] == 16 and on["risk"] is True and on["risk_margin"] == 4
    ev = ["eval", "-m", "x.wt", "-d", "imgs"]
    off, on = vars(parser.parse_args(ev)), vars(parser.parse_args(ev + ["--risk"]))
    assert off["risk"] is False and on["risk"] is True and on["risk_margin"] == 16 and on["ssim"] is False and on["calibration"] is False
    tr = ["train", "start", "-a", "ssdn", "--noise_style", "gauss25", "--noise_value", "known", "-t", "imgs", "-i", "64"]
    off = vars(parser.parse_args(tr + ["--noisy"]))
    on = vars(parser.parse_args(tr + ["--noisy", "--noisy_validation", "held_out"]))
    assert off["noisy_validation"] is None and on["noisy_validation"] == "held_out" and on["noisy"] == "style"
    texts = {}
    for act in parser._actions:
        for name, p in (getattr(act, "choices", None) or {}).items():
            if hasattr(p, "format_help"):
                texts[name] = " ".join(p.format_help().split())
    assert "--risk" in texts["denoise"] and "too large reads as a better PSNR" in texts["denoise"] and "--risk_margin" in texts["denoise"]
    assert "--risk" in texts["eval"] and "risk.csv" in texts["eval"]


def test_denoise_refusals_before_any_device_work(tmp_path):
    """impulse and n2c models, and risk with tile=: raised from the configuration alone, on CPU-built models"""
    from ssdn.__main__ import start_cli
    imp = _cpu_denoiser(style="impulse50")
    with pytest.raises(NotImplementedError, match="impulse model: its posterior mean is not affine in the pixel and its noise is not zero-mean"):
        imp.denoise([], noise_param=50, risk=True)
    with pytest.raises(NotImplementedError, match="impulse"):
        imp.risk([])
    n2c = _cpu_denoiser("n2c")
    with pytest.raises(NotImplementedError, match="mse pipeline has no reference-free risk estimate.*ssdn_u_only.*divergence"):
        n2c.denoise([], risk=True)
    ok = _cpu_denoiser()
    with pytest.raises(ValueError, match="risk=True with tile= is not supported: overlapping tiles would count pixels twice"):
        ok.denoise([], noise_param=25, risk=True, tile=64)
    with pytest.raises(ValueError, match="risk_margin must be at least 0"):
        ok.denoise([], noise_param=25, risk=True, risk_margin=-2)
    assert ok.denoise([], noise_param=25, risk=True) == {"out": [], "noise_std": [], "risk": []}
    assert ok.denoise([], noise_param=25) == {"out": [], "noise_std": []}              # without the flag: the dict of today
    ok.check_risk()
    _cpu_denoiser(style="poisson30", value="var").check_risk()
    # the commands refuse the same models after loading them and before anything is written
    _save(imp, tmp_path / "imp.wt")
    _save(n2c, tmp_path / "n2c.wt")
    with pytest.raises(NotImplementedError, match="impulse"):
        start_cli(["denoise", "-m", str(tmp_path / "imp.wt"), "-i", str(tmp_path / "none"), "-o", str(tmp_path / "out"), "--noise_param", "50", "--risk"])
    with pytest.raises(ValueError, match="--risk: the mse pipeline has no reference-free risk estimate"):
        start_cli(["eval", "-m", str(tmp_path / "n2c.wt"), "-d", str(tmp_path / "none"), "--runs_dir", str(tmp_path / "runs"), "--risk"])
    assert not os.path.exists(tmp_path / "out") and not os.path.exists(tmp_path / "runs")


def test_denoise_csv_header_with_and_without_the_flag(tmp_path, monkeypatch):
    """the command's file around a stand-in for Denoiser.denoise: four more columns and a last log line with --risk, the header and the
    call of today without"""
    import logging
    from PIL import Image
    from ssdn.__main__ import start_cli
    from ssdn.denoiser import Denoiser
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    for i in range(3):
        Image.fromarray(np.full((8, 9, 3), 40 * i, dtype=np.uint8)).save(imgs / ("im%d.png" % i))
    _save(_cpu_denoiser(), tmp_path / "model.wt")
    calls = []

    def fake(self, images, **kw):
        calls.append(kw)
        res = {"out": [torch.zeros(8, 9, 3, dtype=torch.uint8) for _ in images], "noise_std": [0.1] * len(images)}
        if kw.get("risk"):
            res["risk"] = [dict({k: 0.5 for k in VALUES}, psnr_out_est=v, psnr_mu_est=20.25, nll=-1.5, clipped=0.125)
                           for v in (30.5, float("nan"), 31.5)][:len(images)]
        return res
    monkeypatch.setattr(Denoiser, "denoise", fake)
    records = []
    handler = logging.Handler()
    handler.emit = lambda rec: records.append(rec.getMessage())
    logging.getLogger("ssdn.denoise").addHandler(handler)
    logging.getLogger("ssdn.denoise").setLevel(logging.INFO)
    try:
        base = ["denoise", "-m", str(tmp_path / "model.wt"), "-i", str(imgs), "--noise_param", "25"]
        start_cli(base + ["-o", str(tmp_path / "off")])
        assert all("risk" not in kw and "risk_margin" not in kw for kw in calls) and not records
        start_cli(base + ["-o", str(tmp_path / "on"), "--risk", "--risk_margin", "3"])
    finally:
        logging.getLogger("ssdn.denoise").removeHandler(handler)
    assert calls[-1]["risk"] is True and calls[-1]["risk_margin"] == 3
    off = open(tmp_path / "off" / "denoise.csv").read().splitlines()
    on = open(tmp_path / "on" / "denoise.csv").read().splitlines()
    assert off[0] == "file,width,height,noise_std" and on[0] == off[0] + ",psnr_out_est,psnr_mu_est,nll,clipped"
    assert [ln.rsplit(",", 4)[0] for ln in on[1:]] == off[1:]
    assert on[1].endswith(",30.500000,20.250000,-1.500000,0.125000") and on[2].endswith(",nan,20.250000,-1.500000,0.125000")
    assert len(records) == 1 and "psnr_out_est=31.0000" in records[0] and "2 of 3 images" in records[0] and "1 without an estimate" in records[0]


def test_check_noisy_and_the_trainers_switches():
    import ssdn
    from ssdn.denoiser import Denoiser
    from ssdn.params import ConfigValue, NoiseAlgorithm, NoiseValue
    from ssdn.train import RISK_METRICS, DenoiserTrainer, check_noisy

    def cfg(algorithm="ssdn", style="gauss25"):
        c = ssdn.cfg.base()
        c[ConfigValue.ALGORITHM] = NoiseAlgorithm(algorithm)
        c[ConfigValue.NOISE_STYLE] = style
        if algorithm == "ssdn":
            c[ConfigValue.NOISE_VALUE] = NoiseValue.KNOWN
        c[ConfigValue.TRAIN_PATCH_SIZE] = 32
        return ssdn.cfg.infer(c, model_only=True)
    with pytest.raises(ValueError, match="--noisy_validation .* needs --noisy"):
        check_noisy(cfg(), None, validation="held_out")
    check_noisy(cfg(), "style", validation="held_out")
    check_noisy(cfg(), None)
    tr = DenoiserTrainer(cfg())
    assert tr.risk is False and tr.risk_margin == 16 and tr.noisy_validation is None
    assert not any("risk" in v.name.lower() for v in ConfigValue)
    assert RISK_METRICS == (("psnr_out_est", "psnr_out_est"), ("psnr_mu_est", "psnr_mu_est"), ("nll_noisy", "nll"))
    # the `.training` key: only when set; a loaded file restores it
    tr.denoiser = Denoiser(tr.cfg, device="cpu")
    tr.init_state()
    tr.noisy = "style"
    assert tr.state_dict()["noisy"] == {"mode": "style", "augment": False, "pool_bytes": None}
    tr.noisy_validation = "held_out"
    sd = tr.state_dict()
    assert sd["noisy"] == {"mode": "style", "augment": False, "pool_bytes": None, "validation": "held_out"}
    back = DenoiserTrainer(cfg())
    back.load_state_dict(sd)
    assert back.noisy == "style" and back.noisy_validation == "held_out"
    tr.noisy_validation = None
    back.load_state_dict(tr.state_dict())
    assert back.noisy_validation is None
    # without --noisy, and for a model without the estimate: refused when training starts, before an image is read
    tr.noisy, tr.noisy_validation = None, "held_out"
    with pytest.raises(ValueError, match="needs --noisy"):
        tr._load_noisy_validation()
    imp = DenoiserTrainer(cfg(style="impulse50"))
    imp.denoiser = Denoiser(imp.cfg, device="cpu")
    imp.noisy, imp.noisy_validation = "style", "held_out"
    with pytest.raises(NotImplementedError, match="--noisy_validation: no reference-free risk estimate for an impulse model"):
        imp._load_noisy_validation()
    n2v = DenoiserTrainer(cfg("n2v"))
    n2v.denoiser = Denoiser(n2v.cfg, device="cpu")
    n2v.noisy, n2v.noisy_validation = "style", "held_out"
    with pytest.raises(NotImplementedError, match="--noisy_validation: the .* pipeline has no reference-free risk estimate"):
        n2v._load_noisy_validation()
    # the noise parameter the held-out images are denoised with, as the training mode has it
    assert tr._noisy_validation_param() == 25
    tr.noisy = "auto"
    assert tr._noisy_validation_param() == "auto"
    tr.cfg[ConfigValue.NOISE_VALUE] = NoiseValue.UNKNOWN_CONSTANT
    assert tr._noisy_validation_param() is None
    # NaN estimates stay out of the means
    hist = ssdn.utils.MetricDict()
    DenoiserTrainer._add_risk(hist, {"psnr_out_est": [30.0, float("nan"), 32.0], "psnr_mu_est": [float("nan")], "nll": [-1.0, -2.0]})
    assert float(torch.as_tensor(hist["psnr_out_est"].accumulated()).mean()) == 31.0 and hist["psnr_mu_est"].empty()
    assert float(torch.as_tensor(hist["nll_noisy"].accumulated()).mean()) == -1.5
