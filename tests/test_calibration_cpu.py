"""CPU: posterior calibration (ssdn.utils.calculate_calibration, SSDN_OP_CALIBRATION, `ssdn eval --calibration`): the float64 specification
by hand, against numpy.linalg and against the statistics of samples drawn from the posterior itself, its named constants, the C ABI of the
op and its argument rules (raised before any device call, so they show without a GPU), and the opt-in switches of the trainer and the
command line."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from calib_ref import CHI2, TRI, calib_numpy, make_inputs
from ssdn.hip import lib as L
from ssdn.utils import calculate_calibration
from ssdn.utils import data as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUES = ["nll", "maha", "rmse_ratio", "cover_1s", "cover_2s", "cover_3s", "cover_50", "cover_90", "cover_99", "degenerate"]


# ---- 1. the specification -------------------------------------------------------------------------------------------------------------------
def test_one_channel_by_hand():
    """mean 0, cov 4, ref 2: z = 1, d2 = 1, logdet = ln 4, and `<=` counts the equality"""
    res = calculate_calibration(torch.zeros(1, 1, 1, 1), torch.full((1, 1, 1, 1), 4.0), torch.full((1, 1, 1, 1), 2.0), hist=True, zmap=True)
    assert set(res) == set(VALUES) | {"stats", "hist", "zmap"}
    s = res["stats"]
    assert s.dtype == torch.float64 and tuple(s.shape) == (1, 12)
    #                       N  deg d2  logdet       |r|^2 tr  1s 2s 3s  50 90 99     (d2 = 1 lies above the median 0.4549 of chi^2_1)
    assert s[0].tolist() == [1, 0, 1.0, float(s[0, 3]), 4.0, 4.0, 1, 1, 1, 0, 1, 1] and abs(float(s[0, 3]) - math.log(4.0)) <= 1e-15
    assert float(res["zmap"]) == 1.0 and res["zmap"].shape == (1, 1, 1, 1)
    hist = res["hist"]
    assert hist.dtype == torch.int64 and tuple(hist.shape) == (1, 1, 34) and int(hist.sum()) == 1 and int(hist[0, 0, 1 + 20]) == 1    # floor(4 * 1 + 16)
    assert float(res["maha"]) == 1.0 and float(res["rmse_ratio"]) == 1.0 and float(res["cover_1s"]) == 1.0 and float(res["cover_50"]) == 0.0
    assert abs(float(res["nll"]) - (0.5 * (1.0 + math.log(4.0)) + 0.5 * math.log(2 * math.pi))) <= 1e-15 and float(res["degenerate"]) == 0.0
    # the tails and the first inner bin of the histogram
    for zv, b in ((-4.5, 0), (-4.0, 1), (-3.76, 1), (3.99, 32), (4.0, 33), (17.0, 33), (-0.01, 16), (0.0, 17)):
        h = calculate_calibration(torch.zeros(1, 1, 1, 1), torch.ones(1, 1, 1, 1), torch.full((1, 1, 1, 1), zv), hist=True)["hist"]
        assert int(h[0, 0, b]) == 1 and int(h.sum()) == 1, (zv, b)


@pytest.mark.parametrize("Cn", [1, 3])
def test_against_numpy_linalg(Cn):
    mean, cov, ref = make_inputs(2, Cn, 9, 13, seed=Cn)
    res = calculate_calibration(mean, cov, ref, hist=True, zmap=True)
    d2, logdet, z = calib_numpy(mean, cov, ref)
    s = res["stats"].numpy()
    n = 9 * 13
    r = ref.double().numpy() - mean.double().numpy()
    diag = [k for k, (i, j) in enumerate(TRI) if i == j] if Cn == 3 else [0]
    want = {0: np.full(2, n), 1: np.zeros(2), 2: d2.sum((1, 2)), 3: logdet.sum((1, 2)), 4: (r * r).sum((1, 2, 3)),
            5: cov.double().numpy()[:, diag].sum((1, 2, 3))}
    for k, lvl in enumerate((1.0, 2.0, 3.0)):
        want[6 + k] = (np.abs(z) <= lvl).sum((1, 2, 3))
    for k, q in enumerate(CHI2[Cn]):
        want[9 + k] = (d2 <= q).sum((1, 2))
    for k, w in want.items():
        if k in (2, 3, 4, 5):
            np.testing.assert_allclose(s[:, k], w, rtol=1e-9, atol=0, err_msg="statistic %d" % k)
        else:
            assert (s[:, k] == w).all(), (k, s[:, k], w)
    np.testing.assert_allclose(res["zmap"].numpy(), z, rtol=1e-9, atol=0)
    bins = np.where(z < -4, 0, np.where(z >= 4, 33, 1 + np.floor(4 * z + 16))).astype(np.int64)
    for b in range(2):
        for c in range(Cn):
            assert (res["hist"][b, c].numpy() == np.bincount(bins[b, c].ravel(), minlength=34)).all()
    # the reported values from the raw statistics
    nc = n * Cn
    np.testing.assert_allclose(res["nll"].numpy(), 0.5 * (s[:, 2] + s[:, 3]) / nc + 0.5 * math.log(2 * math.pi), rtol=1e-15)
    np.testing.assert_allclose(res["maha"].numpy(), s[:, 2] / nc, rtol=1e-15)
    np.testing.assert_allclose(res["rmse_ratio"].numpy(), np.sqrt(s[:, 4] / s[:, 5]), rtol=1e-15)
    for k, name in enumerate(("cover_1s", "cover_2s", "cover_3s")):
        np.testing.assert_allclose(res[name].numpy(), s[:, 6 + k] / nc, rtol=1e-15)
    for k, name in enumerate(("cover_50", "cover_90", "cover_99")):
        np.testing.assert_allclose(res[name].numpy(), s[:, 9 + k] / n, rtol=1e-15)
    # the counts are spread: the builder's z-scores and distances reach every threshold
    assert (0 < s[:, 6]).all() and (s[:, 6] < s[:, 7]).all() and (s[:, 7] <= s[:, 8]).all() and (s[:, 8] <= nc).all()
    assert (0 < s[:, 9]).all() and (s[:, 9] < s[:, 10]).all() and (s[:, 10] <= s[:, 11]).all()


def test_chi2_constants_against_the_closed_form_cdfs():
    cdf = {1: lambda x: math.erf(math.sqrt(x / 2)),
           3: lambda x: math.erf(math.sqrt(x / 2)) - math.sqrt(2 * x / math.pi) * math.exp(-x / 2)}
    assert D.CALIB_CHI2_LEVELS == (0.5, 0.9, 0.99) and D.CALIB_CHI2 == CHI2
    for Cn in (1, 3):
        for p, q in zip(D.CALIB_CHI2_LEVELS, D.CALIB_CHI2[Cn]):
            assert abs(cdf[Cn](q) - p) <= 1e-12, (Cn, p, q, cdf[Cn](q))
    for k, lvl in zip((1, 2, 3), D.CALIB_SIGMA_LEVELS):
        assert abs(math.erf(k / math.sqrt(2)) - lvl) <= 1e-15
    assert ["%.6f" % v for v in D.CALIB_SIGMA_LEVELS] == ["0.682689", "0.954500", "0.997300"]
    # the header's copies
    hdr = open(os.path.join(ROOT, "include", "ssdn_hip.h")).read()
    for Cn in (1, 3):
        m = re.search(r"#define SSDN_CALIB_CHI2_C%d \{([^}]*)\}" % Cn, hdr)
        assert tuple(float(v) for v in m.group(1).split(",")) == CHI2[Cn]


def test_samples_of_the_posterior_itself_are_calibrated():
    """ref = mean + L g on a 64 x 64 x 3 field: N = 4096 independent pixels.
    A pixel-level coverage (cover_50/90/99) is a binomial share of N trials: sd = sqrt(p (1 - p) / N).  A channel-level coverage
    (cover_1s/2s/3s) is the mean over N independent pixels of the share of a pixel's 3 correlated channels inside the band, a variable in
    [0, 1] with mean p and variance at most p (1 - p): the same sd bounds it.  d2 is chi^2_3 (mean 3, variance 6), so maha = sum d2 / (3 N)
    has sd sqrt(2 / (3 N)).  |r|^2 of a pixel has mean tr S and variance 2 tr(S^2) <= 2 (tr S)^2, so rmse_ratio^2 = sum |r|^2 / sum tr S has
    sd at most eps = sqrt(2 sum (tr S)^2) / sum tr S.  Every value must lie within 5 of its sd of the nominal one.  With the covariance
    scaled by 1/4 (exact in floating point) d2 is exactly 4 times larger and the predicted variance 4 times smaller: maha = 4 and
    rmse_ratio^2 = 4 within 4 times the same bounds."""
    g = torch.Generator().manual_seed(20261019)
    H = W = 64
    N, Cn = H * W, 3
    A = (torch.rand(1, H, W, 3, 3, generator=g, dtype=torch.float64) * 2 - 1) * 0.05
    S = A @ A.transpose(-1, -2) + 1e-4 * torch.eye(3, dtype=torch.float64)
    mean = torch.rand(1, 3, H, W, generator=g, dtype=torch.float64)
    z = torch.randn(1, H, W, 3, 1, generator=g, dtype=torch.float64)
    ref = mean + (torch.linalg.cholesky(S) @ z)[..., 0].permute(0, 3, 1, 2)
    cov = torch.stack([S[..., i, j] for i, j in TRI], 1)
    tr = S.diagonal(dim1=-2, dim2=-1).sum(-1)
    eps = float(torch.sqrt(2 * (tr * tr).sum()) / tr.sum())
    res = calculate_calibration(mean, cov, ref)
    assert float(res["stats"][0, 0]) == N and float(res["degenerate"]) == 0.0
    nominal = dict(zip(("cover_1s", "cover_2s", "cover_3s"), D.CALIB_SIGMA_LEVELS))
    nominal.update(zip(("cover_50", "cover_90", "cover_99"), D.CALIB_CHI2_LEVELS))
    for name, p in nominal.items():
        sd = math.sqrt(p * (1 - p) / N)
        print("%s: %.5f, nominal %.5f, %.2f sd" % (name, float(res[name]), p, (float(res[name]) - p) / sd))
        assert abs(float(res[name]) - p) <= 5 * sd, name
    sd_m = math.sqrt(2.0 / (N * Cn))
    print("maha %.5f (%.2f sd), rmse_ratio %.5f (ratio^2 - 1 = %.2f eps)" % (float(res["maha"]), (float(res["maha"]) - 1) / sd_m,
                                                                            float(res["rmse_ratio"]), (float(res["rmse_ratio"]) ** 2 - 1) / eps))
    assert abs(float(res["maha"]) - 1) <= 5 * sd_m
    assert abs(float(res["rmse_ratio"]) ** 2 - 1) <= 5 * eps
    # an over-confident model: the covariance four times too small
    over = calculate_calibration(mean, cov / 4, ref)
    assert abs(float(over["maha"]) - 4) <= 4 * 5 * sd_m and abs(float(over["rmse_ratio"]) ** 2 - 4) <= 4 * 5 * eps
    assert abs(float(over["maha"]) - 4 * float(res["maha"])) <= 1e-12 and abs(float(over["rmse_ratio"]) - 2 * float(res["rmse_ratio"])) <= 1e-12
    assert float(over["cover_2s"]) < nominal["cover_2s"] - 0.2 and float(over["cover_90"]) < 0.6 and float(over["nll"]) > float(res["nll"])


def test_degenerate_pixels_are_counted_and_left_out():
    mean, cov, ref = make_inputs(2, 3, 6, 7, seed=7)
    base = calculate_calibration(mean, cov, ref, hist=True, zmap=True)
    mean, cov, ref = mean.clone(), cov.clone(), ref.clone()
    cov[0, :, 1, 2] = 0.0                                                          # an all-zero covariance
    mean[0, 1, 3, 3] = float("nan")                                                # a NaN
    ref[0, 2, 0, 0] = float("inf")
    cov[0, :, 4, 5] = torch.tensor([1.0, 1.0, 0.0, 1.0, 0.0, 1.0])                 # the exact singular [[1,1,0],[1,1,0],[0,0,1]]: p1 = 0
    cov[0, :, 5, 6] = torch.tensor([1.0, 0.0, 0.0, -1.0, 0.0, 1.0])                # a negative variance
    cov[0, 4, 2, 2] = float("nan")                                                 # a NaN off the diagonal
    bad = [(1, 2), (3, 3), (0, 0), (4, 5), (5, 6), (2, 2)]
    res = calculate_calibration(mean, cov, ref, hist=True, zmap=True)
    keep = torch.ones(6, 7, dtype=torch.bool)
    for i, j in bad:
        keep[i, j] = False
    # sample 0 is what its valid pixels alone give (laid out as a 1 x 36 image); sample 1 is untouched
    alone = calculate_calibration(mean[:1, :, keep][:, :, None], cov[:1, :, keep][:, :, None], ref[:1, :, keep][:, :, None], hist=True)
    s = res["stats"]
    assert s[0, 0] == 36 and s[0, 1] == 6 and float(res["degenerate"][0]) == 6 / 42
    assert torch.equal(s[0, [0, 6, 7, 8, 9, 10, 11]], alone["stats"][0, [0, 6, 7, 8, 9, 10, 11]]) and torch.equal(res["hist"][0], alone["hist"][0])
    assert torch.allclose(s[0, 2:6], alone["stats"][0, 2:6], rtol=1e-12, atol=0) and torch.isfinite(s).all()
    for k in VALUES[:-1]:
        assert abs(float(res[k][0]) - float(alone[k][0])) <= 1e-12 * abs(float(alone[k][0])), k
    assert torch.equal(torch.isnan(res["zmap"][0]), ~keep[None].expand(3, 6, 7))
    assert torch.equal(s[1], base["stats"][1]) and torch.equal(res["hist"][1], base["hist"][1]) and torch.equal(res["zmap"][1], base["zmap"][1])
    # no valid pixel at all: the ratios are NaN, the counts stay
    none = calculate_calibration(mean[:1, :, :1, :1], torch.zeros(1, 6, 1, 1), ref[:1, :, :1, :1], hist=True)
    assert none["stats"][0].tolist() == [0, 1] + [0] * 10 and int(none["hist"].sum()) == 0
    assert all(math.isnan(float(none[k])) for k in VALUES[:-1]) and float(none["degenerate"]) == 1.0


def test_shapes_are_checked():
    m, c, r = make_inputs(1, 3, 4, 5)
    for bad in ((m[:, :2], c, r[:, :2]), (m, c[:, :5], r), (m[0], c[0], r[0]), (m, c, r[:, :, :3])):
        with pytest.raises(ValueError, match="calculate_calibration"):
            calculate_calibration(*bad)


# ---- 2. the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_struct_size():
    hdr = open(os.path.join(ROOT, "include", "ssdn_hip.h")).read()
    assert re.search(r"SSDN_OP_CALIBRATION\s*=\s*28\b", hdr) and "} ssdn_calibration_args;" in hdr
    assert re.search(r"#define SSDN_ABI_VERSION 19\b", hdr) and L.ABI_VERSION == 19
    assert L.OP["calibration"] == 28 and L.ARG_TYPES["calibration"] is L.CalibrationArgs
    assert [n for n, _ in L.CalibrationArgs._fields_] == ["mean", "cov", "ref", "ext", "B", "C", "H", "W", "stats", "hist", "zmap", "scratch",
                                                          "scratch_bytes"]
    assert L.load().ssdn_struct_size(28) == C.sizeof(L.CalibrationArgs)
    # the scratch rule of the header and the binding's copy of it
    blk, ns, nb = (int(re.search(r"#define SSDN_CALIB_%s (\d+)" % a, hdr).group(1)) for a in ("BLOCK", "NSTATS", "HIST_BINS"))
    assert (blk, ns, nb) == (L.CALIB_BLOCK, L.CALIB_NSTATS, L.CALIB_HIST_BINS) == (256, 12, 34) == (256, D.CALIB_NSTATS, D.CALIB_HIST_BINS)
    assert L.calib_scratch_bytes(2, 3, 8, 8) == 96 * 2 and L.calib_scratch_bytes(3, 3, 37, 70) == 96 * 3 * 11 and L.calib_scratch_bytes(1, 1, 16, 16) == 96


def _refused(**kw):
    """run one op with dummy (never dereferenced) pointers -> the library's error text"""
    f = dict(mean=0x1000, cov=0x1000, ref=0x1000, ext=None, B=1, C=3, H=16, W=16, stats=0x1000, hist=None, zmap=None, scratch=0x1000,
             scratch_bytes=1 << 20)
    f.update(kw)
    a = L.CalibrationArgs(**f)
    rec = (L.OpRec * 1)()
    rec[0].type, rec[0].lane, rec[0].args = L.OP["calibration"], 0, C.cast(C.pointer(a), C.c_void_p)
    lib = L.load()
    assert lib.ssdn_run_ops(rec, 1, None) != 0
    return lib.ssdn_last_error().decode()


@pytest.mark.parametrize("kw,msg", [
    (dict(mean=None), "mean, cov and ref must be given"),
    (dict(cov=None), "mean, cov and ref must be given"),
    (dict(ref=None), "mean, cov and ref must be given"),
    (dict(stats=None), "the output stats must be given"),
    (dict(C=2), "C must be 1 or 3"),
    (dict(C=0), "C must be 1 or 3"),
    (dict(C=4), "C must be 1 or 3"),
    (dict(B=0), "B, H and W must be at least 1"),
    (dict(H=0), "B, H and W must be at least 1"),
    (dict(W=-1), "B, H and W must be at least 1"),
    (dict(scratch=None), "scratch must be given"),
    (dict(scratch_bytes=95), "scratch_bytes is below"),
    (dict(H=17, scratch_bytes=96), "scratch_bytes is below"),
    (dict(scratch=0x1004), "scratch must be 8-byte aligned"),
    (dict(B=65536, scratch_bytes=1 << 40), "B must be at most 65535"),
    (dict(H=1 << 16, W=1 << 15, scratch_bytes=1 << 40), "H \\* W at most"),
])
def test_run_ops_refuses_bad_arguments_without_a_gpu(kw, msg):
    err = _refused(**kw)
    assert re.search(r"^op 0 \(type 28\): calibration: .*" + msg, err), err


# ---- 3. the switches ------------------------------------------------------------------------------------------------------------------------
def test_cli_eval_calibration_flag():
    from ssdn.cli.cli import build_parser
    parser, _ = build_parser()
    on = vars(parser.parse_args(["eval", "-m", "x.wt", "-d", "imgs", "--calibration"]))
    off = vars(parser.parse_args(["eval", "-m", "x.wt", "-d", "imgs"]))
    assert on["calibration"] is True and off["calibration"] is False and on["ssim"] is False
    assert vars(parser.parse_args(["eval", "-m", "x.wt", "-d", "imgs", "--calibration", "--ssim"]))["ssim"] is True


def test_cli_refuses_a_model_without_a_posterior(tmp_path):
    """--calibration with an MSE model: an error after the model is loaded and before anything runs (no run directory appears)"""
    import ssdn
    from ssdn.__main__ import start_cli
    from ssdn.denoiser import Denoiser
    from ssdn.params import ConfigValue, NoiseAlgorithm
    cfg = ssdn.cfg.base()
    cfg[ConfigValue.ALGORITHM] = NoiseAlgorithm.NOISE_TO_CLEAN
    cfg[ConfigValue.NOISE_STYLE] = "gauss25"
    d = Denoiser(ssdn.cfg.infer(cfg, model_only=True), device="cpu")
    torch.save({k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in d.state_dict().items()}, tmp_path / "model.wt")
    with pytest.raises(ValueError, match="--calibration: the mse pipeline has no posterior covariance"):
        start_cli(["eval", "-m", str(tmp_path / "model.wt"), "-d", str(tmp_path / "none"), "--runs_dir", str(tmp_path / "runs"), "--calibration"])
    assert not os.path.exists(tmp_path / "runs")


def test_trainer_switch_is_off_by_default_and_no_config_value():
    from ssdn.params import ConfigValue
    from ssdn.train import DenoiserTrainer
    tr = DenoiserTrainer({})
    assert tr.calibration is False and tr.calibration_hist is None
    assert not any("calib" in v.name.lower() for v in ConfigValue)


def test_planned_lists_know_nothing_of_the_op():
    for f in (("selfsupervised-denoising_amd", "ssdn", "hip", "graph.py"), ("oracle", "interp.py")):
        assert "calibration" not in open(os.path.join(ROOT, *f)).read().lower()


def test_trainer_cpu_path_is_the_specification_on_the_unpadded_triples():
    """DenoiserTrainer.calculate_calibration without a GPU: calculate_calibration on each un-padded (mean, cov, clean) triple; an MSE
    trainer refuses"""
    import ssdn
    from ssdn.datasets import NoisyDataset
    from ssdn.params import ConfigValue, NoiseAlgorithm, NoiseValue, PipelineOutput
    from ssdn.train import _POSTERIOR_COV, DenoiserTrainer
    MD = NoisyDataset.Metadata
    cfg = ssdn.cfg.base()
    cfg[ConfigValue.ALGORITHM] = NoiseAlgorithm.SELFSUPERVISED_DENOISING
    cfg[ConfigValue.NOISE_STYLE] = "gauss25"
    cfg[ConfigValue.NOISE_VALUE] = NoiseValue.KNOWN
    tr = DenoiserTrainer(ssdn.cfg.infer(cfg, model_only=True))
    mean, cov, ref = make_inputs(2, 3, 32, 32, seed=3)
    meta = {MD.CLEAN: ref, MD.IMAGE_SHAPE: torch.tensor([[3, 32, 32], [3, 20, 13]])}
    got = tr.calculate_calibration([mean, ref, meta], {PipelineOutput.IMG_DENOISED: mean, _POSTERIOR_COV: cov})
    want = [calculate_calibration(mean[:1], cov[:1], ref[:1], hist=True),
            calculate_calibration(mean[1:, :, :20, :13], cov[1:, :, :20, :13], ref[1:, :, :20, :13], hist=True)]
    assert set(got) == set(VALUES) | {"stats", "hist"}
    for k in got:
        assert torch.equal(got[k], torch.cat([w[k] for w in want])), k
    assert got["stats"][1, 0] == 20 * 13
    cfg = ssdn.cfg.base()
    cfg[ConfigValue.ALGORITHM] = NoiseAlgorithm.NOISE_TO_CLEAN
    cfg[ConfigValue.NOISE_STYLE] = "gauss25"
    with pytest.raises(NotImplementedError, match="mse pipeline"):
        DenoiserTrainer(ssdn.cfg.infer(cfg, model_only=True)).calculate_calibration([mean, ref, meta], {PipelineOutput.IMG_DENOISED: mean})
