"""GPU: SSDN_OP_CALIBRATION (csrc/calibration.hip) against the float64 specification ssdn.utils.calculate_calibration, the bits it promises,
its degenerate-pixel and extent rules, Denoiser.calibration and `ssdn eval --calibration`.

Bounds.  The counts (statistics 0, 1, 6..11) and the histogram are compared exactly: the op-level inputs come from calib_ref.make_inputs,
which asserts that no value lies within 1e-9 (relative) of a threshold it is counted against.  The four sums (statistics 2..5) agree at
rtol 1e-9: both sides are fp64, the condition number is at most 1e4 and a sample has at most a few thousand terms, so the bound is
~n * 2^-53 * cond << 1e-9.  A z-map value is the float64 value rounded once to fp32: rtol 1.2e-7.

The shapes.  A workgroup takes 256 pixels of a sample's extent, numbered row-major over the extent.  (2,3,8,8) and (2,1,5,7) are one partial
workgroup per sample; (3,3,37,70) with the extents (37,70), (1,1) and (20,33) has samples of 2590 pixels = 10 full workgroups and one of 30
pixels, of one pixel, and of 660 pixels = 2 full workgroups and one of 148 pixels, in a grid of 11 workgroups per sample, so the second and
third sample also have workgroups that lie wholly outside their extent."""
import os

import numpy as np
import pytest
import torch

import restate as R
from calib_ref import make_inputs
from head_ops import DEV, P, run_one
from ssdn.utils import calculate_calibration

pytestmark = pytest.mark.gpu
COUNTS, SUMS = [0, 1, 6, 7, 8, 9, 10, 11], [2, 3, 4, 5]
RTOL_SUM, RTOL_MAP = 1e-9, 1.2e-7
VALUES = ["nll", "maha", "rmse_ratio", "cover_1s", "cover_2s", "cover_3s", "cover_50", "cover_90", "cover_99", "degenerate"]

SHAPES = [(2, 3, 8, 8, None), (2, 1, 5, 7, None), (3, 3, 37, 70, [(37, 70), (1, 1), (20, 33)])]


def calib_op(mean, cov, ref, ext=None, want_hist=True, want_map=True, map_init=None):
    """one SSDN_OP_CALIBRATION launch on device copies -> (stats [B,12] float64, hist [B,C,34] int64 or None, zmap [B,C,H,W] or None), host
    tensors.  stats is NaN before the launch, hist holds garbage (the op zeroes it), zmap is NaN unless map_init is given, and the scratch
    holds garbage of its own"""
    from ssdn.hip import lib as L
    B, C, H, W = mean.shape
    md, cd, rd = (t.to(DEV, torch.float32).contiguous() for t in (mean, cov, ref))
    ed = torch.tensor(ext, dtype=torch.int32, device=DEV).contiguous() if ext is not None else None
    stats = torch.full((B, 12), float("nan"), dtype=torch.float64, device=DEV)
    hist = torch.full((B, C, 34), 123456789, dtype=torch.int64, device=DEV) if want_hist else None
    zmap = (torch.full((B, C, H, W), float("nan"), device=DEV) if map_init is None else map_init.to(DEV).clone()) if want_map else None
    nbytes = L.calib_scratch_bytes(B, C, H, W)
    scratch = torch.full((nbytes // 8,), 1e300, dtype=torch.float64, device=DEV)
    run_one("calibration", L.CalibrationArgs(P(md), P(cd), P(rd), P(ed), B, C, H, W, P(stats), P(hist), P(zmap), P(scratch), nbytes))
    return stats.cpu(), (hist.cpu() if want_hist else None), (zmap.cpu() if want_map else None)


_CASES = {}


def case(i):
    """inputs, one launch with histogram and map and the specification of shape i: computed once, shared, never modified"""
    if i not in _CASES:
        B, C, H, W, ext = SHAPES[i]
        mean, cov, ref = make_inputs(B, C, H, W, seed=10 + i)
        stats, hist, zmap = calib_op(mean, cov, ref, ext)
        exts = ext if ext is not None else [(H, W)] * B
        spec = [calculate_calibration(mean[b:b + 1, :, :e1, :e2], cov[b:b + 1, :, :e1, :e2], ref[b:b + 1, :, :e1, :e2], hist=True, zmap=True)
                for b, (e1, e2) in enumerate(exts)]
        _CASES[i] = dict(mean=mean, cov=cov, ref=ref, ext=ext, exts=exts, stats=stats, hist=hist, zmap=zmap, spec=spec)
    return _CASES[i]


def check_against(stats, hist, zmap, spec, e1, e2, what):
    """one sample of the op against the specification of its cropped inputs; prints every figure before it asserts"""
    want = spec["stats"][0]
    rel = ((stats[SUMS] - want[SUMS]).abs() / want[SUMS].abs()).tolist()
    got_map, want_map = zmap[:, :e1, :e2].double(), spec["zmap"][0]
    ok = torch.isfinite(want_map)
    merr = float(((got_map[ok] - want_map[ok]).abs() / want_map[ok].abs().clamp_min(1e-300)).max()) if bool(ok.any()) else 0.0
    print("%s: counts %s (spec %s), sums rel err %s, z-map rel err %.3e, hist diff %d"
          % (what, stats[COUNTS].tolist(), want[COUNTS].tolist(), ["%.2e" % r for r in rel], merr, int((hist - spec["hist"][0]).abs().sum())))
    assert torch.equal(stats[COUNTS], want[COUNTS]), what
    assert torch.equal(hist, spec["hist"][0]), what
    assert max(rel) <= RTOL_SUM, what
    assert torch.equal(torch.isnan(got_map), ~ok) and merr <= RTOL_MAP, what


# ---- 1. the op against the definition ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_op_against_the_float64_specification(i):
    c = case(i)
    for b, (e1, e2) in enumerate(c["exts"]):
        check_against(c["stats"][b], c["hist"][b], c["zmap"][b], c["spec"][b], e1, e2, "shape %s sample %d" % (SHAPES[i][:4], b))
        assert c["stats"][b, 0] == e1 * e2 and c["stats"][b, 1] == 0
        outside = torch.ones(c["zmap"].shape[1:], dtype=torch.bool)
        outside[:, :e1, :e2] = False
        assert torch.isnan(c["zmap"][b][outside]).all() and torch.isfinite(c["zmap"][b, :, :e1, :e2]).all()        # written inside the extent only


# ---- 2. the bits it promises -----------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return torch.equal(a.nan_to_num(nan=7.0), b.nan_to_num(nan=7.0))


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_bits_repeat_with_and_without_outputs_and_whatever_the_padding(i):
    c = case(i)
    B, C, H, W = SHAPES[i][:4]
    stats, hist, zmap = calib_op(c["mean"], c["cov"], c["ref"], c["ext"])
    assert torch.equal(stats, c["stats"]) and torch.equal(hist, c["hist"]) and _same(zmap, c["zmap"])
    for wh, wm in ((False, False), (True, False), (False, True)):
        s2, h2, m2 = calib_op(c["mean"], c["cov"], c["ref"], c["ext"], want_hist=wh, want_map=wm)
        assert torch.equal(s2, c["stats"]) and (h2 is None or torch.equal(h2, c["hist"])) and (m2 is None or _same(m2, c["zmap"]))
    # a z-map that held numbers keeps them outside the extents
    init = torch.full(c["zmap"].shape, 3.0)
    _, _, kept = calib_op(c["mean"], c["cov"], c["ref"], c["ext"], map_init=init)
    inside = torch.zeros(c["zmap"].shape, dtype=torch.bool)
    for b, (e1, e2) in enumerate(c["exts"]):
        inside[b, :, :e1, :e2] = True
    assert torch.equal(kept, torch.where(inside, c["zmap"], init))
    # other padding: the same extents inside a larger tensor whose remainder holds NaN, a zero covariance and huge values
    Hp, Wp = H + 5, W + 27
    big = []
    for t, fill in ((c["mean"], float("nan")), (c["cov"], 0.0), (c["ref"], 1e30)):
        p = torch.full((B, t.shape[1], Hp, Wp), fill)
        for b, (e1, e2) in enumerate(c["exts"]):
            p[b, :, :e1, :e2] = t[b, :, :e1, :e2]
        big.append(p)
    s3, h3, m3 = calib_op(*big, [list(e) for e in c["exts"]])
    assert torch.equal(s3, c["stats"]) and torch.equal(h3, c["hist"])
    for b, (e1, e2) in enumerate(c["exts"]):
        assert torch.equal(m3[b, :, :e1, :e2], c["zmap"][b, :, :e1, :e2])
        # sample b alone, un-padded and contiguous
        crop = [t[b:b + 1, :, :e1, :e2] for t in (c["mean"], c["cov"], c["ref"])]
        s4, h4, m4 = calib_op(*crop)
        assert torch.equal(s4[0], c["stats"][b]) and torch.equal(h4[0], c["hist"][b]) and torch.equal(m4[0], c["zmap"][b, :, :e1, :e2]), b


# ---- 3. degenerate pixels, clamped and empty extents ---------------------------------------------------------------------------------------
def test_degenerate_pixels_clamped_and_empty_extents():
    c = case(2)
    mean, cov, ref = c["mean"].clone(), c["cov"].clone(), c["ref"].clone()
    # sample 0 (37 x 70): degenerate pixels in the first, a middle and the last (partial) workgroup
    cov[0, :, 0, 3] = 0.0                                                          # an all-zero covariance
    mean[0, 1, 17, 40] = float("nan")                                              # a NaN
    ref[0, 0, 20, 0] = float("inf")
    cov[0, :, 36, 69] = torch.tensor([1.0, 1.0, 0.0, 1.0, 0.0, 1.0])               # the exact singular [[1,1,0],[1,1,0],[0,0,1]]
    cov[0, :, 36, 50] = torch.tensor([1.0, 0.0, 0.0, 1.0, 0.0, -1.0])              # a negative variance
    cov[0, 1, 5, 5] = float("nan")
    bad = [(0, 3), (17, 40), (20, 0), (36, 69), (36, 50), (5, 5)]
    ext = [[37, 70], [-3, 40], [20, 33]]                                           # sample 1: an empty extent
    stats, hist, zmap = calib_op(mean, cov, ref, ext, map_init=torch.full(c["zmap"].shape, 3.0))
    spec = calculate_calibration(mean[:1], cov[:1], ref[:1], hist=True, zmap=True)
    check_against(stats[0], hist[0], zmap[0], spec, 37, 70, "planted degenerate pixels")
    assert stats[0, 0] == 37 * 70 - 6 and stats[0, 1] == 6 and torch.isfinite(stats).all()
    nan_at = torch.isnan(zmap[0]).any(0).nonzero().tolist()
    assert sorted(map(tuple, nan_at)) == sorted(bad) and torch.isnan(zmap[0]).all(0).sum() == 6
    assert not stats[1].any() and not hist[1].any() and bool((zmap[1] == 3.0).all())            # the empty extent: zeros, nothing of the map
    assert torch.equal(stats[2], c["stats"][2]) and torch.equal(hist[2], c["hist"][2])
    assert torch.equal(zmap[2, :, :20, :33], c["zmap"][2, :, :20, :33])
    # extents outside the tensor are clamped to it by the kernel (ext is device memory)
    s2, h2, m2 = calib_op(c["mean"], c["cov"], c["ref"], [[1000, 1000], [1, 1], [20, 33]])
    assert torch.equal(s2, c["stats"]) and torch.equal(h2, c["hist"]) and _same(m2, c["zmap"])
    s3, _, _ = calib_op(c["mean"], c["cov"], c["ref"], [[37, 70], [1, 1], [0, 0]], want_hist=False, want_map=False)
    assert torch.equal(s3[:2], c["stats"][:2]) and not s3[2].any()


# ---- Denoiser.calibration ---------------------------------------------------------------------------------------------------------------------
SIZES = [(40, 24), (32, 32)]                       # un-padded extents of the two images; the batch is padded to 64 x 64
NPV = {"gauss25": 25 / 255.0, "poisson30": 30.0, "impulse50": 0.5}
# (style, mode, channels, diagonal covariance)
DEN_CASES = [("gauss25", "known", 3, False), ("gauss25", "known", 3, True), ("gauss25", "const", 1, False), ("poisson30", "var", 3, False),
             ("impulse50", "const", 3, False)]


def _denoiser(style, mode, ch, diag=False):
    """blind-spot Denoiser, main network from R.make_params(seed 5), sigma network (var) from seed 6, learnt constant (const) at 1.7"""
    from ssdn.denoiser import Denoiser
    from test_impulse_cpu import impulse_cfg
    d = Denoiser(impulse_cfg(style, mode, ch, diag), device="cuda:0")
    net = d.get_model(Denoiser.MODEL, False)
    net.load_state_dict(R.reference_state_dict(R.make_params(ch, net.state_dict()["output_block.4.bias"].shape[0], True, seed=5)))
    if mode == "var":
        d.get_model(Denoiser.SIGMA_ESTIMATOR, False).load_state_dict(R.reference_state_dict(R.make_params(ch, 1, False, seed=6)))
    if mode == "const":
        with torch.no_grad():
            d.l_params[Denoiser.ESTIMATED_SIGMA].fill_(1.7)
    d.mark_dirty()
    return d


def _eval_batch(style="gauss25", ch=3, seed=0, S=64):
    """a two-image evaluation batch as the padded test loader hands it out: images stored top-left, IMAGE_SHAPE metadata"""
    from ssdn.datasets import NoisyDataset
    MD = NoisyDataset.Metadata
    clean = R.hash_tensor((2, ch, S, S), 161 + seed, 0, 1)
    noisy = torch.clamp(clean + R.hash_tensor((2, ch, S, S), 162 + seed, -1, 1) * 0.17, 0, 1)
    meta = {MD.CLEAN: clean, MD.INPUT_NOISE_VALUES: torch.full((2, 1, 1, 1), NPV[style]),
            MD.IMAGE_SHAPE: torch.tensor([[ch, h, w] for h, w in SIZES]), MD.INDEXES: torch.tensor([0, 1])}
    return [noisy.to(DEV), clean.to(DEV), meta]


@pytest.mark.parametrize("style,mode,ch,diag", DEN_CASES)
def test_denoiser_calibration_is_the_specification_on_the_posterior(style, mode, ch, diag):
    from ssdn.datasets import NoisyDataset
    d = _denoiser(style, mode, ch, diag)
    data = _eval_batch(style, ch)
    with pytest.raises(RuntimeError, match="preceding run_pipeline"):
        d.calibration(data)
    d.eval()
    with torch.no_grad():
        d.run_pipeline(data)
    res = d.calibration(data, hist=True, maps=True)
    assert set(res) == set(VALUES) | {"stats", "hist", "zmap"}
    assert all(res[k].dtype == torch.float64 and res[k].device.type == "cpu" and tuple(res[k].shape) == (2,) for k in VALUES)
    assert tuple(res["stats"].shape) == (2, 12) and res["hist"].dtype == torch.int64 and tuple(res["hist"].shape) == (2, ch, 34)
    assert tuple(res["zmap"].shape) == (2, ch, 64, 64)
    assert set(d.calibration(data)) == set(VALUES) | {"stats"}
    post = d.posterior(data)
    clean = data[2][NoisyDataset.Metadata.CLEAN]
    for b, (h, w) in enumerate(SIZES):
        spec = calculate_calibration(post["mean"][b:b + 1, :, :h, :w].cpu(), post["cov"][b:b + 1, :, :h, :w].cpu(), clean[b:b + 1, :, :h, :w],
                                     hist=True, zmap=True)
        what = "%s %s C=%d diag=%d sample %d" % (style, mode, ch, diag, b)
        print("%s: degenerate %g, %s" % (what, float(res["degenerate"][b]), ", ".join("%s %.4f" % (k, float(res[k][b])) for k in VALUES[:-1])))
        check_against(res["stats"][b], res["hist"][b], res["zmap"][b], spec, h, w, what)
        for k in VALUES:
            assert abs(float(res[k][b]) - float(spec[k][0])) <= RTOL_SUM * abs(float(spec[k][0])), k
        assert float(res["degenerate"][b]) == 0.0 and res["stats"][b, 0] == h * w
        outside = torch.ones(ch, 64, 64, dtype=torch.bool)
        outside[:, :h, :w] = False
        assert torch.isnan(res["zmap"][b][outside]).all()
    # refusals: no clean image; a batch of another shape
    MD = NoisyDataset.Metadata
    with pytest.raises(ValueError, match="no clean image"):
        d.calibration([data[0], data[1], {k: v for k, v in data[2].items() if k != MD.CLEAN}])
    other = dict(data[2])
    other[MD.CLEAN] = data[2][MD.CLEAN][:, :, :32, :32]
    with pytest.raises(ValueError, match="not the last run's shape"):
        d.calibration([data[0], data[1], other])


def test_denoiser_calibration_changes_nothing_else():
    """IMG_DENOISED of the last run, the metric accumulator, the plan blob, the last engines, a following ssim() and accumulate_metrics(): bit
    for bit what they are without the call"""
    from ssdn.params import PipelineOutput as PO

    def run(with_calibration):
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
        if with_calibration:
            d.calibration(data, hist=True, maps=True)
            d.calibration(data)
        assert (d._last_engine, d._last_train_engine) == last and eng.export_plan() == blob
        assert d.read_metrics("keep", reset=False) == before and torch.equal(eng.pme, first)
        ssim = d.ssim(data, maps=True)
        per = d.accumulate_metrics(data, "eval", with_loss=False, per_sample=True)
        d.accumulate_metrics(data, "keep", with_loss=False)
        acc = d.read_metrics("keep")
        with torch.no_grad():
            second = d.run_pipeline(data)[PO.IMG_DENOISED].clone()
        assert torch.equal(first, second)
        return first, ssim, per, acc, d.flat.detach().clone()
    f0, s0, p0, a0, w0 = run(False)
    f1, s1, p1, a1, w1 = run(True)
    assert torch.equal(f0, f1) and all(_same(s0[k], s1[k]) for k in s0) and all(torch.equal(p0[k], p1[k]) for k in p0)
    assert a0 == a1 and torch.equal(w0, w1)


def test_an_mse_denoiser_has_no_calibration():
    import ssdn
    from ssdn.denoiser import Denoiser
    from ssdn.params import ConfigValue, NoiseAlgorithm
    cfg = ssdn.cfg.base()
    cfg[ConfigValue.ALGORITHM] = NoiseAlgorithm.NOISE_TO_CLEAN
    cfg[ConfigValue.NOISE_STYLE] = "gauss25"
    d = Denoiser(ssdn.cfg.infer(cfg, model_only=True), device="cuda:0")
    with pytest.raises(NotImplementedError, match="mse pipeline"):
        d.calibration(_eval_batch())


# ---- `ssdn eval --calibration` ---------------------------------------------------------------------------------------------------------------
def test_cli_eval_calibration_writes_its_files_and_changes_nothing_without_the_flag(tmp_path):
    """`ssdn eval` over a folder of two images, one of them non-square, once with --calibration and once without (loader workers off: their
    start-up is most of an evaluation this small)"""
    import math
    from PIL import Image
    from ssdn.__main__ import start_cli
    from ssdn.eval import DenoiserEvaluator
    from ssdn.params import ConfigValue
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    for i, (w, h) in enumerate([(40, 24), (32, 32)]):
        a = (R.hash_tensor((h, w, 3), 700 + i, 0, 1).numpy() * 255).astype(np.uint8)
        Image.fromarray(a, mode="RGB").save(imgs / ("im%d.png" % i))
    d = _denoiser("gauss25", "known", 3)
    d.cfg[ConfigValue.DATALOADER_WORKERS] = 0
    torch.save({k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in d.state_dict().items()}, tmp_path / "model.wt")
    results = []
    orig = DenoiserEvaluator.evaluate
    base = ["eval", "-m", str(tmp_path / "model.wt"), "-d", str(imgs), "--batch_size", "2"]
    try:
        DenoiserEvaluator.evaluate = lambda self: results.append(orig(self)) or results[-1]
        torch.manual_seed(77)                  # (the loader draws the evaluation noise from torch's host generator: the same for both runs)
        ev = start_cli(base + ["--runs_dir", str(tmp_path / "runs_on"), "--calibration"])
        line = ev.eval_state_str("EVALUATION RESULT")
        # the evaluator's engine still holds that batch: Denoiser.calibration against the loader's clean images and extents
        again = ev.denoiser.calibration(next(iter(ev.testloader)), hist=True)
        torch.manual_seed(77)
        off = start_cli(base + ["--runs_dir", str(tmp_path / "runs_off")])
    finally:
        DenoiserEvaluator.evaluate = orig
    with open(os.path.join(ev.run_dir_path, "calibration.csv")) as fh:
        assert fh.readline() == ",".join(["id"] + VALUES) + "\n"
        raw = [ln.strip().split(",") for ln in fh]
    assert [r[0] for r in raw] == ["0000", "0001"]
    for i, r in enumerate(raw):
        assert r[1:] == ["%.6f" % float(again[k][i]) for k in VALUES], (r, i)
    vals = np.array([[float(v) for v in r[1:]] for r in raw])
    assert np.isfinite(vals).all() and (vals[:, -1] == 0).all()
    with open(os.path.join(ev.run_dir_path, "calibration_hist.csv")) as fh:
        assert fh.readline() == "bin_lo,bin_hi,expected,ch0,ch1,ch2\n"
        rows = [[float(v) for v in ln.strip().split(",")] for ln in fh]
    assert len(rows) == 34 and rows[0][:2] == [-math.inf, -4.0] and rows[1][:2] == [-4.0, -3.75] and rows[33][:2] == [4.0, math.inf]
    cols = np.array(rows)
    assert np.abs(cols[:, 2:].sum(0) - 1).max() <= 34 * 5e-9                        # (eight printed decimals per bin)
    total = again["hist"].sum(0).double()
    assert np.abs(cols[:, 3:] - (total / total.sum(1, keepdim=True)).numpy().T).max() <= 5e-9
    res = results[0]
    for k, name in (("calib_nll", "nll"), ("calib_maha", "maha"), ("calib_rmse_ratio", "rmse_ratio"), ("calib_cover_2s", "cover_2s")):
        mean = float(again[name].mean())
        assert abs(res[k] - mean) <= 1e-6 * abs(mean) and "%s=%8.4f" % (k, res[k]) in line, (k, line)
    # without the flag: neither file, the keys of today, the same psnrs.csv
    assert set(results[1]) == {"psnr_out", "psnr_mu_out"} and set(res) == set(results[1]) | {"calib_nll", "calib_maha", "calib_rmse_ratio", "calib_cover_2s"}
    assert not os.path.exists(os.path.join(off.run_dir_path, "calibration.csv")) and not os.path.exists(os.path.join(off.run_dir_path, "calibration_hist.csv"))
    assert "calib" not in off.eval_state_str("EVALUATION RESULT")
    assert open(os.path.join(ev.run_dir_path, "psnrs.csv"), "rb").read() == open(os.path.join(off.run_dir_path, "psnrs.csv"), "rb").read()
    assert all(results[0][k] == results[1][k] for k in results[1])
