"""No GPU: the float64 definition `ssdn.utils.estimate_noise` against the numpy model of tests/noise_est_ref.py (the table integer for integer,
the floating outputs to 1e-12 relative), its accuracy on a synthetic picture, the C ABI of SSDN_OP_NOISE_EST and its host-side refusals,
and what `Denoiser.denoise(noise_param="auto")`, `Denoiser.estimate_noise` and `ssdn denoise` decide before any device work."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import noise_est_ref as R
from ssdn.hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-12                    # a handful of float64 operations per value, in the same order on both sides


def _same(d, hist, ssum, e):
    """the definition's dict `d` against the model's table and estimates"""
    assert d["hist"].dtype == d["ssum"].dtype == torch.int64 and tuple(d["hist"].shape) == (8, 1024) and tuple(d["ssum"].shape) == (8,)
    assert np.array_equal(d["hist"].numpy(), hist) and np.array_equal(d["ssum"].numpy(), ssum)
    assert (d["n"], d["classes_used"]) == (e["n"], e["classes_used"]) and isinstance(d["n"], int)
    for k in ("sigma", "lambda"):
        assert isinstance(d[k], float) and R.close(d[k], e[k], RTOL), (k, d[k], e[k])
    for k in ("nlf_sigma", "nlf_mean"):
        assert d[k].dtype == torch.float64 and R.close(d[k].numpy(), e[k], RTOL), (k, d[k], e[k])


# ---- 1. the definition against the model ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("h,w", R.SIZES)
def test_table_and_estimates_are_the_models(h, w, Cn):
    from ssdn.utils import estimate_noise
    im = R.make_images([(h, w)], Cn, seed=7 * h + w + Cn)[0]
    hist, ssum, e = R.estimate(im)
    assert e["n"] == hist.sum() <= max(h - 2, 0) * max(w - 2, 0) * Cn
    if h >= 63:                                                     # (enough windows: the estimate exists and several classes are kept)
        assert e["n"] > 2000 and e["classes_used"] >= 5 and 10 < e["sigma"] < 14 and math.isfinite(e["lambda"])
    else:
        assert e["classes_used"] == 0 and math.isnan(e["lambda"])
    _same(estimate_noise(im, hist=True), hist, ssum, e)
    _same(estimate_noise(torch.from_numpy(im), hist=True), hist, ssum, e)
    if Cn == 1:                                                     # [h, w] is [h, w, 1]
        _same(estimate_noise(im[:, :, 0], hist=True), hist, ssum, e)
    assert set(estimate_noise(im)) == {"sigma", "lambda", "n", "classes_used", "nlf_sigma", "nlf_mean"}


@pytest.mark.parametrize("Cn", [1, 3])
def test_saturated_constant_and_checkerboard_images(Cn):
    from ssdn.utils import estimate_noise
    h, w = 40, 44
    # all 255: no valid window, everything NaN
    im = np.full((h, w, Cn), 255, dtype=np.uint8)
    d = estimate_noise(im, hist=True)
    _same(d, *R.estimate(im))
    assert d["n"] == 0 and d["classes_used"] == 0 and math.isnan(d["sigma"]) and math.isnan(d["lambda"])
    assert torch.isnan(d["nlf_sigma"]).all() and torch.isnan(d["nlf_mean"]).all() and int(d["hist"].sum()) == 0
    # constant 128: every window in bin 0 of class 4 -- the floors give finite positive parameters
    im = np.full((h, w, Cn), 128, dtype=np.uint8)
    d = estimate_noise(im, hist=True)
    _same(d, *R.estimate(im))
    assert d["n"] == (h - 2) * (w - 2) * Cn == int(d["hist"][4, 0]) and d["classes_used"] == 1
    assert d["sigma"] == 0.5 and d["lambda"] == 260100.0 and float(d["nlf_mean"][4]) == 128.0
    assert float(d["nlf_sigma"][4]) == 0.25 / R.C_MED            # (the grouped median of a single bin 0 is 0.25; no floor per class)
    # a 1 / 254 checkerboard: |r| = 2024 everywhere, the clamp bin has no median
    yy, xx = np.indices((h, w))
    im = np.repeat(np.where((yy + xx) % 2 == 0, 1, 254).astype(np.uint8)[:, :, None], Cn, 2)
    d = estimate_noise(im, hist=True)
    _same(d, *R.estimate(im))
    assert d["n"] == (h - 2) * (w - 2) * Cn == int(d["hist"][:, 1023].sum()) and math.isnan(d["sigma"]) and math.isnan(d["lambda"])
    assert sorted(np.flatnonzero(d["hist"].sum(1).numpy())) == [3, 4]       # S = 1021 and 1274: classes 3 and 4


def test_grouped_median_by_hand():
    q = np.zeros(1024, dtype=np.int64)
    q[[2, 3, 5]] = [1, 2, 1]                                        # N = 4, half = 2: cum(2) = 1, cum(3) = 3 >= 2 -> k* = 3
    assert R.grouped_median(q) == 2.5 + 1.0 * (2 - 1) / 2
    q[:] = 0
    q[0] = 3                                                        # bin 0 spans [0, 0.5]
    assert R.grouped_median(q) == 0.5 * 1.5 / 3
    q[1023] = 4
    assert math.isnan(R.grouped_median(q)) and math.isnan(R.grouped_median(np.zeros(1024, dtype=np.int64)))
    from ssdn.utils.data import _grouped_median
    g = np.random.default_rng(0)
    qs = g.integers(0, 50, size=(9, 1024))
    qs[3, 200:] = 0
    qs[4, :] = 0
    qs[4, 1023] = 9
    got = _grouped_median(torch.from_numpy(qs))
    assert R.close(got.numpy(), [R.grouped_median(r) for r in qs], RTOL) and math.isnan(float(got[4]))


# ---- 2. accuracy on the synthetic picture of DESIGN.md section 3.17 ---------------------------------------------------------------------------
_CLEAN = {}


def _clean():
    if "img" not in _CLEAN:
        _CLEAN["img"] = R.synthetic(256, 384)
    return _CLEAN["img"]


@pytest.mark.parametrize("kind,value,bound", [("gauss", 5, 0.04), ("gauss", 10, 0.04), ("gauss", 25, 0.04), ("poisson", 30, 0.10),
                                              ("poisson", 100, 0.10)])
def test_accuracy_on_the_synthetic_picture(kind, value, bound):
    """256 x 384 x 3, seeds 0-2; measured: gauss at most 1.8 % off, true Poisson at most 7.5 %; the bounds leave room for other seeds.
    (gauss 50 reads 7 % low and poisson 10 26 % high, from clipping: recorded in DESIGN.md, not asserted.)"""
    from ssdn.utils import estimate_noise
    for seed in range(3):
        d = estimate_noise(R.add_noise(_clean(), kind, value, seed))
        got = d["sigma"] if kind == "gauss" else d["lambda"]
        print(kind, value, seed, got)
        assert abs(got - value) <= bound * value, (kind, value, seed, got)
        assert d["classes_used"] >= 5


# ---- 3. the C ABI -------------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_struct_size():
    hdr = open(os.path.join(ROOT, "include", "ssdn_hip.h")).read()
    assert re.search(r"SSDN_OP_NOISE_EST\s*=\s*31\b", hdr) and "} ssdn_noise_est_args;" in hdr
    assert re.search(r"#define SSDN_ABI_VERSION 19\b", hdr) and L.ABI_VERSION == 19
    assert L.OP["noise_est"] == 31 and L.ARG_TYPES["noise_est"] is L.NoiseEstArgs
    names = ["src", "src_bytes", "offs", "ext", "B", "C", "H", "W", "kind", "hist", "ssum", "est", "param"]
    assert [n for n, _ in L.NoiseEstArgs._fields_] == names
    body = re.search(r"typedef struct ssdn_noise_est_args \{(.*?)\} ssdn_noise_est_args;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*[,;]", body) == names             # the header's fields, in the binding's order
    lib = L.load()
    assert lib.ssdn_struct_size(31) == C.sizeof(L.NoiseEstArgs) == 88
    assert "NOISE_EST" in set(re.findall(r"SSDN_OP_([A-Z_]+)\s*=", hdr))
    assert (L.NOISE_EST_CLASSES, L.NOISE_EST_BINS, L.NOISE_EST_NEST) == (R.NCLS, R.NBIN, R.NEST)
    for name, v in (("CLASSES", 8), ("BINS", 1024), ("NEST", 20)):
        assert re.search(r"#define SSDN_NOISE_EST_%s %d\b" % (name, v), hdr)


def _refused(**kw):
    """run the op with dummy (never dereferenced) pointers -> the library's error text"""
    f = dict(src=0x1000, src_bytes=64, offs=0x1000, ext=0x1000, B=1, C=3, H=32, W=32, kind=0, hist=0x1000, ssum=0x1000, est=0x1000, param=None)
    f.update(kw)
    a = L.NoiseEstArgs(**f)
    rec = (L.OpRec * 1)()
    rec[0].type, rec[0].lane, rec[0].args = L.OP["noise_est"], 0, C.cast(C.pointer(a), C.c_void_p)
    lib = L.load()
    assert lib.ssdn_run_ops(rec, 1, None) != 0
    return lib.ssdn_last_error().decode()


@pytest.mark.parametrize("kw,msg", [(dict(src=None), "must be given"), (dict(offs=None), "must be given"), (dict(ext=None), "must be given"),
                                    (dict(hist=None), "must be given"), (dict(ssum=None), "must be given"), (dict(est=None), "must be given"),
                                    (dict(C=2), "C must be 1 or 3"), (dict(C=0), "C must be 1 or 3"), (dict(C=4), "C must be 1 or 3"),
                                    (dict(B=0), "B, H and W must be at least 1"), (dict(H=0), "B, H and W must be at least 1"),
                                    (dict(W=-1), "B, H and W must be at least 1"), (dict(src_bytes=-1), "byte count must not be negative"),
                                    (dict(kind=2), "kind must be 0"), (dict(kind=-1), "kind must be 0"),
                                    (dict(hist=0x1004), "16-byte aligned"),
                                    (dict(B=65536), "at most 65535"), (dict(W=32 * 65535 + 1), "at most 65535")])
def test_noise_est_refuses_bad_arguments_without_a_gpu(kw, msg):
    err = _refused(**kw)
    assert re.search(r"^op 0 \(type 31\): noise_est: .*" + msg, err), err


def test_planned_lists_know_nothing_of_the_op():
    for f in (("selfsupervised-denoising_amd", "ssdn", "hip", "graph.py"), ("oracle", "interp.py")):
        assert "noise_est" not in open(os.path.join(ROOT, *f)).read().lower()


# ---- 4. the command and the methods' refusals ------------------------------------------------------------------------------------------------------
def test_cli_takes_auto_and_its_help_names_it():
    from ssdn.cli.cli import build_parser
    parser, cmds = build_parser()
    a = vars(parser.parse_args(["denoise", "-m", "x.wt", "-i", "imgs", "-o", "out", "--noise_param", "auto"]))
    assert a["noise_param"] == "auto"
    sub = next(act for act in parser._actions if getattr(act, "choices", None) and "denoise" in act.choices).choices["denoise"]
    assert "auto" in next(act for act in sub._actions if act.dest == "noise_param").help


def _cpu_denoiser(algorithm, style, value=None, channels=3):
    import ssdn
    from ssdn.denoiser import Denoiser
    from ssdn.params import ConfigValue
    cfg = ssdn.cfg.base()
    cfg[ConfigValue.ALGORITHM] = algorithm
    cfg[ConfigValue.NOISE_STYLE] = style
    cfg[ConfigValue.IMAGE_CHANNELS] = channels
    if value is not None:
        cfg[ConfigValue.NOISE_VALUE] = value
    return Denoiser(ssdn.cfg.infer(cfg, model_only=True), device="cpu")


def _save(d, path):
    torch.save({k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in d.state_dict().items()}, path)


def test_auto_is_accepted_where_a_number_is_and_refused_elsewhere(tmp_path):
    """through `.wt` files built on the CPU, as `ssdn denoise` loads them: denoise([]) decides before any device work"""
    from ssdn.denoiser import Denoiser
    from ssdn.params import NoiseAlgorithm, NoiseValue
    A, K = NoiseAlgorithm.SELFSUPERVISED_DENOISING, NoiseValue.KNOWN
    models = {"gauss": (A, "gauss25", K), "poisson": (A, "poisson30", K), "impulse": (A, "impulse50", K),
              "const": (A, "gauss25", NoiseValue.UNKNOWN_CONSTANT), "n2c": (NoiseAlgorithm.NOISE_TO_CLEAN, "gauss25", None)}
    den = {}
    for name, (alg, style, value) in models.items():
        _save(_cpu_denoiser(alg, style, value), tmp_path / (name + ".wt"))
        den[name] = Denoiser.from_state_dict(torch.load(tmp_path / (name + ".wt"), map_location="cpu", weights_only=False))
    for name in ("gauss", "poisson"):
        assert den[name].denoise([], noise_param="auto") == {"out": [], "noise_std": [], "noise_param": []}
        assert den[name].denoise([], noise_param=" AUTO ") == {"out": [], "noise_std": [], "noise_param": []}
        assert den[name]._noise_param_value("auto") == "auto"
        assert den[name].denoise([], noise_param=25) == {"out": [], "noise_std": []}          # (a number: what it was)
        assert den[name].estimate_noise([]) == []
    with pytest.raises(ValueError, match="no estimator exists for impulse noise"):
        den["impulse"].denoise([], noise_param="auto")
    with pytest.raises(ValueError, match="no estimator exists for impulse noise"):
        den["impulse"].estimate_noise([])
    assert den["impulse"].estimate_noise([], kind="gauss") == []
    for name in ("const", "n2c"):
        with pytest.raises(ValueError, match="this model takes none"):
            den[name].denoise([], noise_param="auto")
    with pytest.raises(ValueError, match="kind must be"):
        den["gauss"].estimate_noise([], kind="impulse")
    with pytest.raises(ValueError, match="has 1 channel"):           # denoise's validation
        den["gauss"].estimate_noise([np.zeros((8, 9), dtype=np.uint8)])
    with pytest.raises(ValueError, match="bucket must be a positive multiple of 32"):
        den["gauss"].estimate_noise([], bucket=48)


def test_cli_refuses_auto_for_an_impulse_model_before_any_device_call(tmp_path):
    from ssdn.__main__ import start_cli
    from ssdn.params import NoiseAlgorithm, NoiseValue
    _save(_cpu_denoiser(NoiseAlgorithm.SELFSUPERVISED_DENOISING, "impulse50", NoiseValue.KNOWN), tmp_path / "impulse.wt")
    _save(_cpu_denoiser(NoiseAlgorithm.SELFSUPERVISED_DENOISING, "gauss25", NoiseValue.UNKNOWN_CONSTANT), tmp_path / "const.wt")
    io = ["-i", str(tmp_path / "none"), "-o", str(tmp_path / "out")]
    with pytest.raises(ValueError, match="no estimator exists for impulse noise"):
        start_cli(["denoise", "-m", str(tmp_path / "impulse.wt"), "--noise_param", "auto"] + io)
    with pytest.raises(ValueError, match="this model takes none"):
        start_cli(["denoise", "-m", str(tmp_path / "const.wt"), "--noise_param", "auto"] + io)
    assert not os.path.exists(tmp_path / "out")


def test_csv_header_without_auto_is_what_it_was(tmp_path, monkeypatch):
    """`ssdn denoise` over an empty folder writes the header alone: with a number it is the parent's line, with auto it gains a column"""
    from ssdn.__main__ import start_cli
    from ssdn.params import NoiseAlgorithm, NoiseValue
    _save(_cpu_denoiser(NoiseAlgorithm.SELFSUPERVISED_DENOISING, "gauss25", NoiseValue.KNOWN), tmp_path / "known.wt")
    _save(_cpu_denoiser(NoiseAlgorithm.NOISE_TO_CLEAN, "gauss25"), tmp_path / "n2c.wt")
    import ssdn.cli.cmds.denoise as cmd
    monkeypatch.setattr(cmd, "find_images", lambda path, recursive=False: (str(path), []))
    header = {}
    for name, model, extra in (("number", "known.wt", ["--noise_param", "25"]), ("auto", "known.wt", ["--noise_param", "auto"]),
                               ("n2c", "n2c.wt", [])):
        out = tmp_path / name
        start_cli(["denoise", "-m", str(tmp_path / model), "-i", str(tmp_path), "-o", str(out)] + extra)
        header[name] = open(out / "denoise.csv").read()
    assert header["number"] == "file,width,height,noise_std\n" and header["n2c"] == "file,width,height\n"
    assert header["auto"] == "file,width,height,noise_std,noise_param\n"
