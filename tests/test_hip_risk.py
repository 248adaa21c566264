"""GPU: SSDN_OP_RISK (csrc/risk.hip) against the numpy model of its definition (risk_ref.py), the bits it promises, its degenerate-pixel,
extent and margin rules, Denoiser.risk, Denoiser.denoise(risk=True) and the two identities on the device's own outputs.

Bounds.  The three counts (statistics 0, 1, 11) are compared exactly.  Each of the nine floating-point sums must agree within
tol * (the sum of its terms' absolute values): both sides are fp64, the model inverts T with numpy.linalg and the kernel with a Cholesky
factor, cond(T) <= 1e4 (asserted by the input builder), so a term differs by ~cond * 2^-53 ~ 1e-12 and tol = 1e-9 holds with room (known
noise).  With a learnt estimate (modes const / var) `est` is an fp32 softplus that may differ in the last place between the device and
numpy: one ulp is 6e-8 of sigma and a few times that in a sum, so tol = 1e-5.  There the scale of a sum goes down to the terms a pixel's
value is made of (risk_ref.stats_from's `wide`): q^2 = (e - s)^2 is a square of a difference that cancels, a last-place change delta of
the estimate moves it by 2 |q| delta |s|, and relative to q^2 itself that is unbounded as q -> 0 (measured on the one-pixel sample of
the third shape: 1.6e-5 of q^2 from one ulp of est), while relative to (e + |s|)^2 it is at most 2 delta.  With a known parameter both
sides compute the same est-free values and the narrower per-pixel scale is kept.

The shapes.  A workgroup takes 256 pixels of a sample's margin-shrunk region, numbered row-major over the region.  (2,3,8,8) and (2,1,5,7)
are one partial workgroup per sample (with margin 3: 2 x 2 pixels, and an empty region); (3,3,37,70) with the extents (37,70), (1,1) and
(20,33) has samples of 10 full workgroups and one of 30 pixels, of one pixel, and of 2 full workgroups and one of 148 pixels in a grid of
11 workgroups per sample, so the second and third sample also have workgroups that lie wholly outside their region."""
import math
import os

import numpy as np
import pytest
import torch

import restate as RS
import risk_ref as R
from head_ops import DEV, P, run_one
from ssdn.utils import calculate_risk, risk_values

pytestmark = pytest.mark.gpu
TOL = {0: 1e-9, 1: 1e-5, 2: 1e-5}
GUARD = -7.25e77

SHAPES = [(2, 3, 8, 8, None), (2, 1, 5, 7, None), (3, 3, 37, 70, [(37, 70), (1, 1), (20, 33)])]
# (shape, style, mode, diag, margin)
OP_CASES = [(i, style, "known", diag, margin) for i in range(3) for style in ("gauss", "poisson") for diag in (False, True)
            for margin in (0, 3) if not (diag and SHAPES[i][1] == 1)]
OP_CASES += [(2, "gauss", "const", False, 0), (2, "gauss", "var", True, 3), (2, "poisson", "const", True, 0), (2, "poisson", "var", False, 3),
             (1, "gauss", "var", False, 0), (1, "poisson", "const", False, 0)]


def risk_op(inp, ext=None, margin=0, check_guards=True):
    """one SSDN_OP_RISK launch on device copies -> stats [B,12] float64 on the host.  stats is 0xFF bytes before the launch, the scratch
    holds 1e300, and a guard row behind each of the two outputs must come back untouched"""
    from ssdn.hip import lib as L
    B, C, H, W = inp["noisy"].shape
    dev = {k: torch.from_numpy(np.ascontiguousarray(inp[k])).to(DEV) for k in ("net_out", "noisy", "pme", "noise_param", "est_raw")}
    ed = torch.tensor(ext, dtype=torch.int32, device=DEV).contiguous() if ext is not None else None
    stats = torch.full((B + 1, 12), GUARD, dtype=torch.float64, device=DEV)
    stats[:B].view(torch.uint8).fill_(0xFF)
    nbytes = L.risk_scratch_bytes(B, C, H, W)
    scratch = torch.full((nbytes // 8 + 12,), 1e300, dtype=torch.float64, device=DEV)
    scratch[nbytes // 8:] = GUARD
    mode = inp["mode"]
    run_one("risk", L.RiskArgs(P(dev["net_out"]), P(dev["noisy"]), P(dev["noise_param"]) if mode == 0 else None,
                               P(dev["est_raw"]) if mode != 0 else None, P(dev["pme"]), P(ed), B, C, H, W, inp["style"], mode, inp["diag"],
                               margin, P(stats), P(scratch), nbytes))
    if check_guards:
        assert bool((stats[B] == GUARD).all()) and bool((scratch[nbytes // 8:] == GUARD).all())
    return stats[:B].cpu()


_CASES = {}


def case(i, style, mode, diag, margin):
    """inputs, one launch and the model of an op case: computed once, shared, never modified"""
    key = (i, style, mode, diag, margin)
    if key not in _CASES:
        B, C, H, W, ext = SHAPES[i]
        inp = R.make_inputs(B, C, H, W, style, mode, diag, seed=10 + i)
        stats = risk_op(inp, ext, margin)
        want, scale, px = R.risk_model(inp["net_out"], inp["noisy"], inp["pme"], inp["noise_param"], inp["est_raw"], inp["style"], inp["mode"],
                                       inp["diag"], ext, margin)
        _CASES[key] = dict(inp=inp, ext=ext, stats=stats, want=want, scale=scale if inp["mode"] == 0 else px["wide"])
    return _CASES[key]


def check_against(stats, want, scale, tol, what):
    """one sample of the op against the model; prints every figure before it asserts -> the largest error relative to its scale"""
    stats, want = np.asarray(stats), np.asarray(want)
    rel = [abs(stats[k] - want[k]) / scale[k] if scale[k] > 0 else abs(stats[k] - want[k]) for k in R.FLOAT_SUMS]
    print("%s: counts %s (model %s), sums err / scale %s" % (what, stats[list(R.COUNTS)].tolist(), want[list(R.COUNTS)].tolist(),
                                                            ["%.2e" % r for r in rel]))
    assert (stats[list(R.COUNTS)] == want[list(R.COUNTS)]).all(), what
    assert np.isfinite(stats).all() and max(rel) <= tol, what
    return max(rel)


# ---- 1. the op against the definition ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i,style,mode,diag,margin", OP_CASES)
def test_op_against_the_numpy_model(i, style, mode, diag, margin):
    c = case(i, style, mode, diag, margin)
    B, C, H, W, ext = SHAPES[i]
    worst = 0.0
    for b in range(B):
        e1, e2 = ext[b] if ext is not None else (H, W)
        worst = max(worst, check_against(c["stats"][b], c["want"][b], c["scale"][b], TOL[c["inp"]["mode"]],
                                         "shape %s %s %s diag=%d margin %d sample %d" % (SHAPES[i][:4], style, mode, diag, margin, b)))
        assert c["stats"][b, 0] == max(e1 - 2 * margin, 0) * max(e2 - 2 * margin, 0) and c["stats"][b, 1] == 0
    print("largest error / scale: %.3e" % worst)


def test_the_definition_agrees_with_the_op_on_the_same_inputs():
    """ssdn.utils.calculate_risk fed with the model's inputs: the kernel spells the same arithmetic, so the per-sample sums agree to the
    summation order (1e-12 of the scale)"""
    for key in ((2, "gauss", "known", False, 3), (2, "poisson", "known", True, 0), (1, "gauss", "known", False, 0)):
        c = case(*key)
        inp = c["inp"]
        Cn = inp["noisy"].shape[1]
        mu, cov, n, v = R.definition_inputs(inp["net_out"], inp["noisy"], inp["noise_param"], inp["est_raw"], Cn, inp["style"], inp["mode"], inp["diag"])
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))      # noqa: E731
        res = calculate_risk(t(inp["noisy"]), t(mu), t(cov), t(inp["pme"]), t(n), t(v), ext=c["ext"], margin=key[4])
        for b in range(inp["noisy"].shape[0]):
            check_against(c["stats"][b], res["stats"][b].numpy(), c["scale"][b], 1e-12, "definition %s sample %d" % (key, b))


# ---- 2. the bits it promises -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [(2, "gauss", "known", False, 3), (2, "poisson", "var", False, 3), (0, "gauss", "known", True, 0),
                                 (1, "poisson", "known", False, 0)])
def test_bits_repeat_whatever_the_padding_and_the_other_samples(key):
    c = case(*key)
    i, margin = key[0], key[4]
    B, C, H, W, ext = SHAPES[i]
    inp = c["inp"]
    assert torch.equal(risk_op(inp, ext, margin), c["stats"])
    exts = ext if ext is not None else [(H, W)] * B
    # other padding: the same extents inside a larger tensor whose remainder holds NaN and huge values
    Hp, Wp = H + 5, W + 27
    big = dict(inp)
    for k, fill in (("net_out", np.nan), ("noisy", 1e30), ("pme", np.nan)):
        p = np.full((B, inp[k].shape[1], Hp, Wp), fill, dtype=np.float32)
        for b, (e1, e2) in enumerate(exts):
            p[b, :, :e1, :e2] = inp[k][b, :, :e1, :e2]
        big[k] = p
    assert torch.equal(risk_op(big, [list(e) for e in exts], margin), c["stats"])
    # sample b alone, un-padded and contiguous
    for b, (e1, e2) in enumerate(exts):
        one = dict(inp, **{k: np.ascontiguousarray(inp[k][b:b + 1, :, :e1, :e2]) for k in ("net_out", "noisy", "pme")})
        one["noise_param"] = inp["noise_param"][b:b + 1]
        one["est_raw"] = inp["est_raw"][b:b + 1] if inp["mode"] == 2 else inp["est_raw"]
        assert torch.equal(risk_op(one, None, margin)[0], c["stats"][b]), b


# ---- 3. degenerate pixels, clamped and empty extents ---------------------------------------------------------------------------------------
def test_degenerate_and_clipped_pixels_clamped_and_empty_extents():
    key = (2, "poisson", "known", False, 0)
    c = case(*key)
    inp = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in c["inp"].items()}
    # sample 0 (37 x 70): degenerate pixels in the first, a middle and the last (partial) workgroup
    inp["net_out"][0, 4, 0, 3] = np.nan                # a NaN in U
    inp["net_out"][0, 1, 17, 40] = np.inf              # an infinite mean
    inp["noisy"][0, 0, 20, 0] = np.inf
    inp["pme"][0, 2, 36, 69] = np.nan
    inp["net_out"][0, 8, 36, 50] = -np.inf
    bad = 5
    inp["noisy"][0, 0, 5, 5], inp["noisy"][0, 2, 5, 5], inp["noisy"][0, 1, 36, 68] = 0.0, 1.0, -0.125          # planted clipped samples
    inp["noisy"][0, 1, 20, 0] = 2.0                                                                              # (a degenerate pixel's: not counted)
    ext = [[37, 70], [-3, 40], [20, 33]]                                                                         # sample 1: an empty extent
    stats = risk_op(inp, ext)
    want, scale, px = R.risk_model(inp["net_out"], inp["noisy"], inp["pme"], inp["noise_param"], inp["est_raw"], 1, 0, 0, ext, 0)
    check_against(stats[0], want[0], scale[0], 1e-9, "planted degenerate pixels")
    assert stats[0, 0] == 37 * 70 - bad and stats[0, 1] == bad
    assert stats[0, 11] >= 3 and want[0, 11] == ((inp["noisy"][0] <= 0) | (inp["noisy"][0] >= 1))[:, px["valid"][0]].sum()
    assert not stats[1].any()                                                                                    # the empty extent: zeros
    assert torch.equal(stats[2], c["stats"][2])
    # a negative lambda makes T indefinite wherever Sigma_x is small against it: every pixel of that sample is degenerate (p0 <= 0)
    lam = c["inp"]["noise_param"].copy()
    lam[1] = -0.5
    neg = dict(c["inp"], noise_param=lam)
    s_neg = risk_op(neg, c["ext"])
    assert s_neg[1].tolist() == [0, 1] + [0] * 10 and torch.equal(s_neg[0], c["stats"][0]) and torch.equal(s_neg[2], c["stats"][2])
    # extents outside the tensor are clamped to it by the kernel (ext is device memory); margins that leave nothing
    assert torch.equal(risk_op(c["inp"], [[1000, 1000], [1, 1], [20, 33]]), c["stats"])
    s3 = risk_op(c["inp"], [[37, 70], [1, 1], [0, 0]])
    assert torch.equal(s3[:2], c["stats"][:2]) and not s3[2].any()
    assert not risk_op(c["inp"], c["ext"], margin=19)[1:].any() and not risk_op(c["inp"], c["ext"], margin=2 ** 31 - 1).any()
    s4 = risk_op(c["inp"], c["ext"], margin=10)
    assert s4[:, 0].tolist() == [17 * 50, 0, 0]


# ---- Denoiser.risk ---------------------------------------------------------------------------------------------------------------------------
SIZES = [(40, 24), (32, 32)]                       # un-padded extents of the two images; the batch is padded to 64 x 64
NPV = {"gauss25": 25 / 255.0, "poisson30": 30.0, "impulse50": 0.5}
# (style, mode, channels, diagonal covariance)
DEN_CASES = [("gauss25", "known", 3, False), ("gauss25", "known", 3, True), ("gauss25", "known", 1, False), ("poisson30", "known", 1, False),
             ("gauss25", "var", 3, False)]


def _denoiser(style, mode, ch, diag=False):
    """blind-spot Denoiser, main network from RS.make_params(seed 5), sigma network (var) from seed 6, learnt constant (const) at 1.7"""
    from ssdn.denoiser import Denoiser
    from test_impulse_cpu import impulse_cfg
    d = Denoiser(impulse_cfg(style, mode, ch, diag), device="cuda:0")
    net = d.get_model(Denoiser.MODEL, False)
    net.load_state_dict(RS.reference_state_dict(RS.make_params(ch, net.state_dict()["output_block.4.bias"].shape[0], True, seed=5)))
    if mode == "var":
        d.get_model(Denoiser.SIGMA_ESTIMATOR, False).load_state_dict(RS.reference_state_dict(RS.make_params(ch, 1, False, seed=6)))
    if mode == "const":
        with torch.no_grad():
            d.l_params[Denoiser.ESTIMATED_SIGMA].fill_(1.7)
    d.mark_dirty()
    return d


def _eval_batch(style="gauss25", ch=3, seed=0, S=64, sizes=SIZES):
    """a two-image evaluation batch as the padded test loader hands it out: images stored top-left, IMAGE_SHAPE metadata"""
    from ssdn.datasets import NoisyDataset
    MD = NoisyDataset.Metadata
    clean = RS.hash_tensor((2, ch, S, S), 161 + seed, 0, 1)
    noisy = torch.clamp(clean + RS.hash_tensor((2, ch, S, S), 162 + seed, -1, 1) * 0.17, 0, 1)
    meta = {MD.CLEAN: clean, MD.INPUT_NOISE_VALUES: torch.full((2, 1, 1, 1), NPV[style]), MD.INDEXES: torch.tensor([0, 1])}
    if sizes is not None:
        meta[MD.IMAGE_SHAPE] = torch.tensor([[ch, h, w] for h, w in sizes])
    return [noisy.to(DEV), clean.to(DEV), meta]


def _engine_inputs(d):
    """what the last forward left in the engine, as the numpy model takes it"""
    from ssdn.denoiser import Denoiser
    from ssdn.hip.engine import MODE, STYLE
    eng = d._last_engine
    if eng.mode == "var":
        est = eng.est_raw.cpu().numpy()
    elif eng.mode == "const":
        est = d.l_params[Denoiser.ESTIMATED_SIGMA].detach().reshape(1).cpu().numpy()
    else:
        est = np.zeros(eng.B, dtype=np.float32)
    return dict(net_out=eng.main.tensor("out32").cpu().numpy(), noisy=eng.inp.cpu().numpy(), pme=eng.pme.cpu().numpy(),
                noise_param=eng.noise_param.cpu().numpy(), est_raw=est, style=STYLE[eng.style], mode=MODE[eng.mode], diag=int(eng.diag))


def _definition_of_engine(d, ext, margin, maps=False):
    inp = _engine_inputs(d)
    Cn = inp["noisy"].shape[1]
    mu, cov, n, v = R.definition_inputs(inp["net_out"], inp["noisy"], inp["noise_param"], inp["est_raw"], Cn, inp["style"], inp["mode"], inp["diag"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))      # noqa: E731
    res = calculate_risk(t(inp["noisy"]), t(mu), t(cov), t(inp["pme"]), t(n), t(v), ext=ext, margin=margin, maps=maps)
    _, scale, px = R.risk_model(inp["net_out"], inp["noisy"], inp["pme"], inp["noise_param"], inp["est_raw"], inp["style"], inp["mode"], inp["diag"],
                                ext, margin)
    return res, (scale if inp["mode"] == 0 else px["wide"]), inp


@pytest.mark.parametrize("style,mode,ch,diag", DEN_CASES)
def test_denoiser_risk_is_the_definition_on_the_engines_tensors(style, mode, ch, diag):
    d = _denoiser(style, mode, ch, diag)
    data = _eval_batch(style, ch)
    with pytest.raises(RuntimeError, match="preceding run_pipeline"):
        d.risk(data)
    d.eval()
    with torch.no_grad():
        d.run_pipeline(data)
    values = list(risk_values(torch.zeros(1, 12), ch))
    for margin in (16, 5, 0):                                    # (the default, 16, leaves nothing of 40 x 24 and of 32 x 32: N = 0, NaN values)
        res = d.risk(data, margin=margin) if margin != 16 else d.risk(data)
        assert set(res) == set(values) | {"stats"} and tuple(res["stats"].shape) == (2, 12)
        assert all(res[k].dtype == torch.float64 and res[k].device.type == "cpu" and tuple(res[k].shape) == (2,) for k in values)
        want, scale, inp = _definition_of_engine(d, SIZES, margin)
        for b, (h, w) in enumerate(SIZES):
            what = "%s %s C=%d diag=%d margin %d sample %d" % (style, mode, ch, diag, margin, b)
            print("%s: %s" % (what, ", ".join("%s %.5g" % (k, float(res[k][b])) for k in values)))
            check_against(res["stats"][b], want["stats"][b].numpy(), scale[b], TOL[inp["mode"]], what)
            assert res["stats"][b, 0] == max(h - 2 * margin, 0) * max(w - 2 * margin, 0) and res["stats"][b, 1] == 0
            assert math.isnan(float(res["psnr_out_est"][b])) == (margin == 16 or not float(res["mse_out_est"][b]) > 0)
            assert math.isnan(float(res["nll"][b])) == (margin == 16)
    # without IMAGE_SHAPE the whole image is the extent
    whole = d.risk(_eval_batch(style, ch, sizes=None), margin=0)
    assert whole["stats"][:, 0].tolist() == [64 * 64] * 2
    with pytest.raises(ValueError, match="margin"):
        d.risk(data, margin=-1)


def test_denoiser_risk_changes_nothing_else():
    """IMG_DENOISED of the last run, the metric accumulator, the plan blob, the last engines, a following calibration() and train_step: bit
    for bit what they are without the call"""
    from ssdn.params import PipelineOutput as PO

    def run(with_risk):
        d = _denoiser("gauss25", "known", 3)
        data = _eval_batch()
        d.eval()
        with torch.no_grad():
            first = d.run_pipeline(data)[PO.IMG_DENOISED].clone()
        eng = d._last_engine
        blob = eng.export_plan()
        d.accumulate_metrics(data, "keep", with_loss=False)
        before = d.read_metrics("keep", reset=False)
        last = (d._last_engine, d._last_train_engine)
        if with_risk:
            d.risk(data)
            d.risk(data, margin=0)
        assert (d._last_engine, d._last_train_engine) == last and eng.export_plan() == blob
        assert d.read_metrics("keep", reset=False) == before and torch.equal(eng.pme, first)
        calib = d.calibration(data, hist=True)
        d.accumulate_metrics(data, "keep", with_loss=False)
        acc = d.read_metrics("keep")
        d.train()
        out = d.train_step(data, lr=3e-4)
        loss = out[PO.LOSS].detach().clone()
        if with_risk:
            d.risk(data)                                         # (behind a training step too: the last forward's tensors)
        torch.cuda.synchronize()
        return first, calib, acc, loss, d.flat.detach().clone()
    f0, c0, a0, l0, w0 = run(False)
    f1, c1, a1, l1, w1 = run(True)
    assert torch.equal(f0, f1) and all(torch.equal(c0[k].nan_to_num(nan=7.0), c1[k].nan_to_num(nan=7.0)) for k in c0)
    assert a0 == a1 and torch.equal(l0, l1) and torch.equal(w0, w1)


def test_models_without_a_risk_estimate_raise():
    import ssdn
    from ssdn.denoiser import Denoiser
    from ssdn.params import ConfigValue, NoiseAlgorithm
    cfg = ssdn.cfg.base()
    cfg[ConfigValue.ALGORITHM] = NoiseAlgorithm.NOISE_TO_CLEAN
    cfg[ConfigValue.NOISE_STYLE] = "gauss25"
    d = Denoiser(ssdn.cfg.infer(cfg, model_only=True), device="cuda:0")
    with pytest.raises(NotImplementedError, match="mse pipeline.*divergence"):
        d.risk(_eval_batch())
    imp = _denoiser("impulse50", "known", 3)
    data = _eval_batch("impulse50")
    imp.eval()
    with torch.no_grad():
        imp.run_pipeline(data)
    with pytest.raises(NotImplementedError, match="impulse.*not affine.*not zero-mean"):
        imp.risk(data)
    with pytest.raises(NotImplementedError, match="not affine"):
        imp._last_engine.risk()
    with pytest.raises(NotImplementedError, match="impulse"):
        imp.denoise([], noise_param=50, risk=True)


# ---- the identity on the device ------------------------------------------------------------------------------------------------------------
def _synthetic(ch, style, seed):
    """two 64 x 64 images of the toy recipe's kind that fill the plan with no padding -> (clean, noisy) float32 [2,ch,64,64]"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(64.0), np.arange(64.0), indexing="ij")
    clean = np.stack([np.stack([np.clip(0.5 + 0.35 * np.sin((xx + 19 * b) / 37) * np.cos((yy + 5 * c) / 53) + 0.1 * np.sin((xx + yy + 7 * c) / 11),
                                        0.05, 0.95) for c in range(ch)]) for b in range(2)])
    noisy = clean + rng.normal(0, 25 / 255, clean.shape) if style == "gauss25" else rng.poisson(30 * clean) / 30.0
    return clean.astype(np.float32), noisy.astype(np.float32)


@pytest.mark.parametrize("style,ch", [("gauss25", 3), ("poisson30", 1)])
def test_the_identities_hold_on_the_devices_own_outputs(style, ch):
    """Random weights, two 64 x 64 images, margin 0, unclipped noise: the device's sum q_out and sum q_mu against sum |out - x|^2 and
    sum |mu - x|^2 computed on the host from the same outputs and the clean image; each lies within 5 sqrt(N) std(d), std(d) from the host
    definition's maps.  (No reflection padding here, so the blind spot is exact and no margin is needed.)"""
    from ssdn.datasets import NoisyDataset
    MD = NoisyDataset.Metadata
    d = _denoiser(style, "known", ch)
    clean, noisy = _synthetic(ch, style, 20261021)
    data = [torch.from_numpy(noisy).to(DEV), torch.from_numpy(clean).to(DEV),
            {MD.CLEAN: torch.from_numpy(clean), MD.INPUT_NOISE_VALUES: torch.full((2, 1, 1, 1), NPV[style]), MD.INDEXES: torch.tensor([0, 1])}]
    d.eval()
    with torch.no_grad():
        d.run_pipeline(data)
    res = d.risk(data, margin=0)
    want, _, inp = _definition_of_engine(d, None, 0, maps=True)
    x = clean.astype(np.float64)
    mu, out = inp["net_out"][:, :ch].astype(np.float64), inp["pme"].astype(np.float64)
    N = 64 * 64
    for b in range(2):
        s = res["stats"][b].numpy()
        assert s[0] == N and s[1] == 0
        for name, est, sq in (("mu", mu, s[4] - s[6]), ("out", out, s[5] + s[7])):
            err = ((est[b] - x[b]) ** 2).sum(0)
            dd = want["q_" + name][b].numpy() - err
            bound = 5 * math.sqrt(N) * dd.std()
            print("%s C=%d image %d %s: sum q %.4f, sum |. - x|^2 %.4f, difference %.4f = %.2f sqrt(N) std(d); psnr est %.2f dB, true %.2f dB"
                  % (style, ch, b, name, sq, err.sum(), sq - err.sum(), (sq - err.sum()) / (math.sqrt(N) * dd.std()),
                     float(res["psnr_%s_est" % name][b]), -10 * math.log10(err.sum() / (N * ch))))
            assert abs(sq - err.sum()) <= bound, (name, b)


# ---- Denoiser.denoise(risk=True) ---------------------------------------------------------------------------------------------------------
def _images(dtype, ch=3):
    sizes = [(24, 40), (64, 64), (50, 33)]                      # (w, h)
    out = []
    for i, (w, h) in enumerate(sizes):
        a = RS.hash_tensor((h, w, ch), 900 + i, 0.1, 0.9).numpy()
        out.append((a * 255).astype(np.uint8) if dtype == np.uint8 else (a * 65535).astype(np.uint16))
    return out


@pytest.mark.parametrize("dtype,param", [(np.uint8, 25), (np.uint8, "auto"), (np.uint16, 25)])
def test_denoise_with_risk_leaves_the_bytes_alone_and_is_denoiser_risk(dtype, param):
    from ssdn.datasets import NoisyDataset
    MD = NoisyDataset.Metadata
    d = _denoiser("gauss25", "known", 3)
    images = _images(dtype)
    plain = d.denoise(images, noise_param=param, batch_size=2, bucket=64, uniform=True)
    got = d.denoise(images, noise_param=param, batch_size=2, bucket=64, uniform=True, risk=True, risk_margin=5)
    assert set(got) == set(plain) | {"risk"} and len(got["risk"]) == 3
    assert all(torch.equal(a, b) and a.dtype == b.dtype for a, b in zip(plain["out"], got["out"]))
    values = list(risk_values(torch.zeros(1, 12), 3))
    assert all(list(r) == values and all(isinstance(v, float) for v in r.values()) for r in got["risk"])
    # Denoiser.risk's route on the same padded batches: [0, 1] and [2], padded to 64 x 64
    for idx in ([0, 1], [2]):
        eng = d._engine(len(idx), 64, 64, False)
        eng.image_in([torch.from_numpy(images[k]) for k in idx], white=None)
        noisy = eng.inp.clone()
        if param == "auto":
            npv = torch.tensor([plain["noise_param"][k] for k in idx], dtype=torch.float32)
        else:
            npv = torch.full((len(idx),), 25 / 255.0)
        meta = {MD.INPUT_NOISE_VALUES: npv.view(-1, 1, 1, 1), MD.IMAGE_SHAPE: torch.tensor([[3, images[k].shape[1], images[k].shape[0]] for k in idx])}
        d.eval()
        with torch.no_grad():
            d.run_pipeline([noisy, torch.zeros(0), meta])
        ref = d.risk([noisy, torch.zeros(0), meta], margin=5)
        for b, k in enumerate(idx):
            print("image %d (%s, %s): %s" % (k, dtype.__name__, param, got["risk"][k]))
            for name in values:
                a, w = got["risk"][k][name], float(ref[name][b])
                assert a == w or (math.isnan(a) and math.isnan(w)), (k, name, a, w)
            assert ref["stats"][b, 0] == (images[k].shape[1] - 10) * (images[k].shape[0] - 10)
    with pytest.raises(ValueError, match="risk=True with tile="):
        d.denoise(images, noise_param=param, risk=True, tile=32)
    with pytest.raises(ValueError, match="risk_margin"):
        d.denoise(images, noise_param=param, risk=True, risk_margin=-1)
    assert d.denoise([], noise_param=param, risk=True)["risk"] == []


# ---- the commands ----------------------------------------------------------------------------------------------------------------------------
FOLDER_SIZES = ((48, 64), (40, 56), (64, 64), (33, 70), (50, 41), (20, 36))      # (h, w); the last has no pixel left at margin 16


def _noisy_folder(path, sizes=FOLDER_SIZES, seed=2):
    from PIL import Image
    os.makedirs(path)
    rs = np.random.RandomState(seed)
    for k, (h, w) in enumerate(sizes):
        yy, xx = np.mgrid[0:h, 0:w]
        base = 0.5 + 0.3 * np.sin(xx / (5.0 + k)) * np.cos(yy / 7.0)
        img = np.stack([base, 1 - base, np.roll(base, 3, 1)], -1) + rs.randn(h, w, 3) * (25 / 255.0)
        Image.fromarray(np.uint8(np.clip(img, 0, 1) * 255)).save(os.path.join(path, "im%d.png" % k))
    return [os.path.join(path, "im%d.png" % k) for k in range(len(sizes))]


def _save_model(d, path):
    from ssdn.params import ConfigValue
    d.cfg[ConfigValue.DATALOADER_WORKERS] = 0
    torch.save({k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in d.state_dict().items()}, path)


def test_cli_denoise_risk_writes_the_columns_and_changes_nothing_else(tmp_path):
    from PIL import Image
    from ssdn.__main__ import start_cli
    files = _noisy_folder(str(tmp_path / "photos"))
    d = _denoiser("gauss25", "known", 3)
    _save_model(d, tmp_path / "model.wt")
    base = ["denoise", "-m", str(tmp_path / "model.wt"), "-i", str(tmp_path / "photos"), "--noise_param", "25", "--batch_size", "2"]
    off = start_cli(base + ["-o", str(tmp_path / "off")])
    on = start_cli(base + ["-o", str(tmp_path / "on"), "--risk", "--risk_margin", "4"])
    assert "risk" not in off and len(on["risk"]) == 6
    api = d.denoise([np.array(Image.open(f)) for f in files], noise_param="25", batch_size=2, risk=True, risk_margin=4)
    rows_off = open(tmp_path / "off" / "denoise.csv").read().splitlines()
    rows_on = open(tmp_path / "on" / "denoise.csv").read().splitlines()
    assert rows_off[0] == "file,width,height,noise_std" and rows_on[0] == rows_off[0] + ",psnr_out_est,psnr_mu_est,nll,clipped"
    for k, (a, b) in enumerate(zip(rows_on[1:], rows_off[1:])):
        assert a.rsplit(",", 4)[0] == b
        assert a.split(",")[-4:] == ["%.6f" % api["risk"][k][c] for c in ("psnr_out_est", "psnr_mu_est", "nll", "clipped")], (k, a)
        name = "im%d.png" % k
        assert open(tmp_path / "on" / name, "rb").read() == open(tmp_path / "off" / name, "rb").read()
    print("\n".join(rows_on))
    vals = np.array([[float(v) for v in r.split(",")[-4:]] for r in rows_on[1:]])
    assert np.isfinite(vals[:, 2:]).all()


def test_cli_eval_risk_writes_its_file_and_changes_nothing_without_the_flag(tmp_path):
    from ssdn.__main__ import start_cli
    from ssdn.eval import DenoiserEvaluator
    _noisy_folder(str(tmp_path / "imgs"), sizes=((24, 40), (32, 32)), seed=4)
    d = _denoiser("gauss25", "known", 3)
    _save_model(d, tmp_path / "model.wt")
    results = []
    orig = DenoiserEvaluator.evaluate
    base = ["eval", "-m", str(tmp_path / "model.wt"), "-d", str(tmp_path / "imgs"), "--batch_size", "2"]
    try:
        DenoiserEvaluator.evaluate = lambda self: results.append(orig(self)) or results[-1]
        torch.manual_seed(77)                  # (the loader draws the evaluation noise from torch's host generator: the same for both runs)
        ev = start_cli(base + ["--runs_dir", str(tmp_path / "runs_on"), "--risk", "--risk_margin", "4"])
        line = ev.eval_state_str("EVALUATION RESULT")
        again = ev.denoiser.risk(next(iter(ev.testloader)), margin=4)          # the evaluator's engine still holds that batch
        torch.manual_seed(77)
        off = start_cli(base + ["--runs_dir", str(tmp_path / "runs_off")])
    finally:
        DenoiserEvaluator.evaluate = orig
    values = list(risk_values(torch.zeros(1, 12), 3))
    with open(os.path.join(ev.run_dir_path, "risk.csv")) as fh:
        assert fh.readline() == ",".join(["id"] + values) + "\n"
        raw = [ln.strip().split(",") for ln in fh]
    assert [r[0] for r in raw] == ["0000", "0001"]
    for i, r in enumerate(raw):
        assert r[1:] == ["%.6f" % float(again[k][i]) for k in values], (r, i)
    res = results[0]
    print(line)
    for k, name in (("psnr_out_est", "psnr_out_est"), ("psnr_mu_est", "psnr_mu_est"), ("nll_noisy", "nll")):
        mean = float(again[name][~torch.isnan(again[name])].mean())
        assert abs(res[k] - mean) <= 1e-6 * abs(mean) and ("%s=%8.4f" if k == "nll_noisy" else "%s=%8.2f") % (k, res[k]) in line, (k, line)
    assert set(results[1]) == {"psnr_out", "psnr_mu_out"} and set(res) == set(results[1]) | {"psnr_out_est", "psnr_mu_est", "nll_noisy"}
    assert not os.path.exists(os.path.join(off.run_dir_path, "risk.csv")) and "_est" not in off.eval_state_str("EVALUATION RESULT")
    assert open(os.path.join(ev.run_dir_path, "psnrs.csv"), "rb").read() == open(os.path.join(off.run_dir_path, "psnrs.csv"), "rb").read()
    assert all(results[0][k] == results[1][k] for k in results[1])


def test_cli_trains_with_a_noisy_validation(tmp_path):
    import glob
    import re
    from ssdn.__main__ import start_cli
    from ssdn.params import ConfigValue, StateValue
    from test_hip_trainer import _scalars
    data, held = str(tmp_path / "photos"), str(tmp_path / "held_out")
    _noisy_folder(data)
    _noisy_folder(held, seed=9)
    base = ["train", "start", "--noisy", "-a", "ssdn", "--noise_value", "known", "-n", "gauss25", "-t", data, "-i", "64", "--train_batch_size", "4",
            "--patch_size", "32", "--print_interval", "32", "--eval_interval", "32", "--checkpoint_interval", "64", "--validation_batch_size", "2"]
    torch.manual_seed(20261021)
    tr = start_cli(base + ["--noisy_validation", held, "--runs_dir", str(tmp_path / "runs_on")])
    torch.manual_seed(20261021)
    off = start_cli(base + ["--runs_dir", str(tmp_path / "runs_off")])
    run = tr.run_dir_path
    assert tr.state[StateValue.ITERATION] == 64 and len(tr._nv_images) == 6
    log = open(os.path.join(run, "log.txt")).read()
    valid = [ln for ln in log.splitlines() if "VALID |" in ln]
    print("\n".join(valid))
    assert len(valid) == 3 and all(re.search(r"psnr_out_est=\s*-?[\d.]+, psnr_mu_est=\s*-?[\d.]+, nll_noisy=\s*-?[\d.]+", ln) for ln in valid)
    sc = _scalars(run)
    assert all([s for s, _ in sc["valid/" + k]] == [0, 32, 64] for k in ("psnr_out_est", "psnr_mu_est", "nll_noisy"))
    assert sorted(os.path.basename(f) for f in glob.glob(os.path.join(run, "val_imgs", "*"))) == ["%08d_noisy-val_out.png" % i for i in (0, 32, 64)]
    sd = torch.load(os.path.join(run, "training", "model_00000064.training"), map_location="cpu", weights_only=False)
    assert sd["noisy"] == {"mode": "style", "augment": False, "pool_bytes": None, "validation": held}
    # the last line's values are the Python API's on the final weights
    api = tr.denoiser.denoise(tr._nv_images, noise_param=25, batch_size=tr.cfg[ConfigValue.TEST_MINIBATCH_SIZE], risk=True)
    assert math.isnan(api["risk"][5]["psnr_out_est"]) and tr.cfg[ConfigValue.TEST_MINIBATCH_SIZE] == 2
    for name, key, fmt in (("psnr_out_est", "psnr_out_est", "%8.2f"), ("psnr_mu_est", "psnr_mu_est", "%8.2f"), ("nll_noisy", "nll", "%8.4f")):
        v = torch.tensor([r[key] for r in api["risk"]], dtype=torch.float64)
        mean = float(v[~torch.isnan(v)].to(torch.float32).mean())
        assert "%s=%s" % (name, fmt % mean) in valid[-1], (name, mean, valid[-1])
    # without the flag: no VALID line, no val_imgs, the key set of today, and the same weights
    log_off = open(os.path.join(off.run_dir_path, "log.txt")).read()
    assert "VALID |" not in log_off and not os.path.exists(os.path.join(off.run_dir_path, "val_imgs"))
    assert not any(k.startswith("valid/") for k in _scalars(off.run_dir_path))
    sd_off = torch.load(os.path.join(off.run_dir_path, "training", "model_00000064.training"), map_location="cpu", weights_only=False)
    assert sd_off["noisy"] == {"mode": "style", "augment": False, "pool_bytes": None}
    assert torch.equal(tr.denoiser.flat, off.denoiser.flat)
    r = __import__("ssdn.train", fromlist=["resume_run"]).resume_run(run)
    assert r.noisy_validation == held
