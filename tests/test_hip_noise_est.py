"""GPU: SSDN_OP_NOISE_EST (csrc/noise_est.hip) against the numpy model of tests/noise_est_ref.py -- the integer table bit for bit, the fp64
estimates to 1e-12 relative --, its guards on inconsistent tables, `Denoiser.estimate_noise` against the host definition,
`Denoiser.denoise(noise_param="auto")` against the same call with the number, what both leave alone, and `ssdn denoise --noise_param auto`.

Tolerances: the table is exact integers.  The estimates are a handful of fp64 operations in the same order on both sides, contraction
off: 1e-12 relative.  The fp32 parameter is one rounding of such a value, so at most one fp32 unit in the last place apart (2^-23)."""
import csv
import math

import numpy as np
import pytest
import torch

import noise_est_ref as R
from head_ops import DEV, P, run_one

pytestmark = pytest.mark.gpu
RTOL = 1e-12
ULP32 = 2.0 ** -23


# ---- 1. the op against the model -----------------------------------------------------------------------------------------------------------------
def noise_est_op(buf, nbytes, offs, ext, Cn, H, W, kind, repeat=1, want_param=True):
    """`repeat` SSDN_OP_NOISE_EST launches on device copies; every output is 0xFF bytes before the first, with 64 such bytes behind each
    -> (hist [B,8,1024] uint32, ssum [B,8] uint64, est [B,20] float64, param [B] float32 or None, the guard bytes behind the outputs)"""
    from ssdn.hip import lib as L
    B = len(offs)
    src = torch.from_numpy(np.ascontiguousarray(buf)).to(DEV)
    od = torch.tensor(offs, dtype=torch.int64, device=DEV)
    ed = torch.tensor(ext, dtype=torch.int32, device=DEV).contiguous()
    sizes = [B * R.NCLS * R.NBIN * 4, B * R.NCLS * 8, B * R.NEST * 8, B * 4]
    outs = [torch.full((n + 64,), 0xFF, dtype=torch.uint8, device=DEV) for n in sizes]
    a = L.NoiseEstArgs(P(src), nbytes, P(od), P(ed), B, Cn, H, W, kind, P(outs[0]), P(outs[1]), P(outs[2]), P(outs[3]) if want_param else None)
    for _ in range(repeat):
        run_one("noise_est", a)
    host = [t.cpu().numpy() for t in outs]
    assert np.array_equal(src.cpu().numpy(), buf)                   # (the input is only read)
    guards = np.concatenate([h[n:] for h, n in zip(host, sizes)])
    hist = host[0][:sizes[0]].view(np.uint32).reshape(B, R.NCLS, R.NBIN)
    ssum = host[1][:sizes[1]].view(np.uint64).reshape(B, R.NCLS)
    est = host[2][:sizes[2]].view(np.float64).reshape(B, R.NEST)
    return hist, ssum, est, (host[3][:sizes[3]].view(np.float32) if want_param else host[3][:sizes[3]]), guards


def _check(got, want, kind):
    hist, ssum, est, par, guards = got
    whist, wssum, west, dicts = want
    assert np.array_equal(hist, whist) and np.array_equal(ssum, wssum)
    assert R.close(est, west, RTOL), (est, west)
    assert np.array_equal(est[:, 2:4], west[:, 2:4])                # n and the classes kept are integers
    wpar = np.array([R.param(e, kind) for e in dicts], dtype=np.float32)
    assert R.close(par, wpar, ULP32), (par, wpar)
    assert (guards == 0xFF).all()


@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("sizes,H,W", [(R.SIZES, 160, 160), (R.SIZES_TILE, 160, 96)], ids=["sizes", "tile_edges"])
def test_op_against_the_numpy_model_bit_for_bit(sizes, H, W, Cn):
    """seven images in one packed buffer with 16 guard bytes of 0xAB between them and a tail; the outputs start as 0xFF bytes; a repeated
    launch gives the same bytes"""
    images = R.make_images(sizes, Cn, seed=10 * H + W + Cn)
    buf, offs = R.pack(images, tail=48)
    ext = [(w, h) for h, w in sizes]
    want = R.noise_est_ref(buf, buf.size, offs, ext, Cn, H, W)
    for b, im in enumerate(images):                                 # (the packed model is the plain definition of every image)
        assert np.array_equal(want[0][b], R.estimate(im)[0])
    assert sum(np.isfinite(want[2][:, 0])) >= 3 and sum(np.isfinite(want[2][:, 1])) >= 3
    got = noise_est_op(buf, buf.size, offs, ext, Cn, H, W, kind=0)
    _check(got, want, 0)
    again = noise_est_op(buf, buf.size, offs, ext, Cn, H, W, kind=0, repeat=2)
    for x, y in zip(got, again):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    _check(noise_est_op(buf, buf.size, offs, ext, Cn, H, W, kind=1), want, 1)
    # without `param` nothing is written there
    none = noise_est_op(buf, buf.size, offs, ext, Cn, H, W, kind=1, want_param=False)
    assert (none[3] == 0xFF).all() and np.array_equal(none[0], want[0]) and R.close(none[2], want[2], RTOL)


@pytest.mark.parametrize("Cn", [1, 3])
def test_special_images_on_the_device(Cn):
    """all 255 (nothing valid: NaN), constant 128 (the floors), the 1 / 254 checkerboard (the clamp bin: NaN)"""
    h, w = 40, 70
    yy, xx = np.indices((h, w))
    images = [np.full((h, w, Cn), 255, dtype=np.uint8), np.full((h, w, Cn), 128, dtype=np.uint8),
              np.repeat(np.where((yy + xx) % 2 == 0, 1, 254).astype(np.uint8)[:, :, None], Cn, 2)]
    buf, offs = R.pack(images)
    ext = [(w, h)] * 3
    want = R.noise_est_ref(buf, buf.size, offs, ext, Cn, 96, 64)
    got = noise_est_op(buf, buf.size, offs, ext, Cn, 96, 64, kind=0)
    _check(got, want, 0)
    est = got[2]
    assert np.isnan(est[0, :2]).all() and est[0, 2] == 0 and np.isnan(got[3][0])
    assert est[1, 0] == 0.5 and est[1, 1] == 260100.0 and got[3][1] == np.float32(0.5 / 255.0)
    assert np.isnan(est[2, :2]).all() and est[2, 2] == (h - 2) * (w - 2) * Cn


def test_inconsistent_tables_are_clamped_and_guarded():
    """The buffers are what the arguments say; only the tables are wrong: extents beyond the tensor or negative, offsets that run past the
    byte count, start behind it or are negative, and a byte count below the buffer's size.  The results are the model's (a byte outside
    is not there, its windows do not count), nothing outside the outputs is written and the launch ends clean."""
    Cn, H, W = 3, 64, 96
    im = R.make_images([(50, 40)], Cn, seed=5)[0]                  # (h, w) = (50, 40)
    buf, offs = R.pack([im] * 6)
    n = buf.size - 2000                                             # the byte count the op is told: the last image straddles it
    ext = [(40, 50), (999, 999), (-3, 50), (40, 50), (40, 50), (40, 50)]
    offs = [offs[0], offs[1], offs[2], n + 4096, -8, offs[5]]
    want = R.noise_est_ref(buf, n, offs, ext, Cn, H, W)
    got = noise_est_op(buf, n, offs, ext, Cn, H, W, kind=0)
    _check(got, want, 0)
    cnt = got[2][:, 2]
    assert cnt[0] > 4000 and cnt[1] > cnt[0] and cnt[2] == cnt[3] == cnt[4] == 0 and 0 < cnt[5] < cnt[0]
    torch.cuda.synchronize()


# ---- 2. the Denoiser's methods ---------------------------------------------------------------------------------------------------------------------
SIZES = [(24, 40), (64, 64), (50, 33)]                               # (h, w)
_DEN = {}


def _model(style, ch):
    """a known-parameter ssdn model with random weights (the constructor's He-normal draw under a fixed seed), built once and shared"""
    if (style, ch) not in _DEN:
        import ssdn
        from ssdn.denoiser import Denoiser
        from ssdn.params import ConfigValue, NoiseAlgorithm, NoiseValue
        cfg = ssdn.cfg.base()
        cfg[ConfigValue.ALGORITHM] = NoiseAlgorithm.SELFSUPERVISED_DENOISING
        cfg[ConfigValue.NOISE_STYLE] = style
        cfg[ConfigValue.IMAGE_CHANNELS] = ch
        cfg[ConfigValue.NOISE_VALUE] = NoiseValue.KNOWN
        torch.manual_seed(11)
        d = Denoiser(ssdn.cfg.infer(cfg, model_only=True), device="cuda:0")
        d.mark_dirty()
        _DEN[(style, ch)] = d
    return _DEN[(style, ch)]


def _images(ch, seed=0):
    """noisy pictures of SIZES whose intensities stay within two classes, so that even 24 x 40 x 1 keeps a class for the Poisson fit"""
    g = np.random.default_rng(200 + seed)
    res = []
    for k, (h, w) in enumerate(SIZES):
        y, x = np.mgrid[0:h, 0:w]
        base = 100.0 + 50.0 * ((x + 2 * y) % 31) / 30.0
        res.append(np.clip(np.rint(base[:, :, None] + g.normal(0, 6.0 + 4 * k, (h, w, ch))), 0, 255).astype(np.uint8))
    return res


def _host_param(d, kind):
    return np.float32(d["sigma"] / 255.0) if kind == "gauss" else np.float32(d["lambda"])


@pytest.mark.parametrize("style,ch", [("gauss25", 3), ("poisson30", 1)])
def test_denoiser_estimate_noise_is_the_host_definition(style, ch):
    from ssdn.utils import estimate_noise
    d = _model(style, ch)
    images = _images(ch)
    keep = (d._last_engine, d._last_train_engine, d.training)
    for kind in (None, "gauss", "poisson"):
        res = d.estimate_noise(images, kind=kind, batch_size=2)
        assert len(res) == 3
        for im, got in zip(images, res):
            want = estimate_noise(im)
            assert set(got) == set(want) | {"noise_param"}
            assert (got["n"], got["classes_used"]) == (want["n"], want["classes_used"]) and want["classes_used"] >= 1
            for k in ("sigma", "lambda"):
                assert math.isfinite(want[k]) and R.close(got[k], want[k], RTOL), (k, got[k], want[k])
            for k in ("nlf_sigma", "nlf_mean"):
                assert R.close(got[k].numpy(), want[k].numpy(), RTOL)
            assert R.close(got["noise_param"], _host_param(want, kind or style[:-2]), ULP32)
    assert (d._last_engine, d._last_train_engine, d.training) == keep
    gray = d.estimate_noise([im[:, :, 0] for im in images]) if ch == 1 else None      # [h, w] arrays, one at a time
    assert gray is None or [g["n"] for g in gray] == [estimate_noise(im)["n"] for im in images]


@pytest.mark.parametrize("uniform", [True, False])
@pytest.mark.parametrize("style,ch", [("gauss25", 3), ("poisson30", 1)])
def test_denoise_auto_is_denoise_with_the_number_byte_for_byte(style, ch, uniform):
    """per image: the same call (the same batches on the same plans) with that image's value as the number gives that image's bytes"""
    from ssdn.utils import estimate_noise
    d = _model(style, ch)
    images = _images(ch, seed=1)
    res = d.denoise(images, noise_param="auto", batch_size=2, uniform=uniform, std=True)
    assert set(res) == {"out", "noise_std", "std", "noise_param"}
    values = res["noise_param"]
    assert all(isinstance(v, float) and v == float(np.float32(v)) for v in values) and len(set(values)) == 3
    for k, im in enumerate(images):
        assert R.close(values[k], _host_param(estimate_noise(im), style[:-2]), ULP32)
        ref = d.denoise(images, noise_param=values[k], batch_size=2, uniform=uniform, std=True)
        assert "noise_param" not in ref
        assert torch.equal(res["out"][k], ref["out"][k]) and len(np.unique(res["out"][k].numpy())) > 8
        assert res["noise_std"][k] == ref["noise_std"][k] and torch.equal(res["std"][k], ref["std"][k])
        other = (k + 1) % 3
        assert not torch.equal(res["out"][other], ref["out"][other])         # (the value matters: another image's output differs)


def test_denoise_auto_names_the_image_without_an_estimate():
    d = _model("gauss25", 3)
    good = _images(3, seed=2)[0]
    with pytest.raises(ValueError, match=r"image 1 has too few valid 3x3 windows"):
        d.denoise([good, np.full((2, 2, 3), 90, dtype=np.uint8)], noise_param="auto")
    with pytest.raises(ValueError, match=r"image 0 has too few valid 3x3 windows"):
        d.denoise([np.full((40, 40, 3), 255, dtype=np.uint8), good], noise_param="auto", batch_size=2, uniform=True)
    assert math.isnan(d.estimate_noise([np.full((2, 2, 3), 90, dtype=np.uint8)])[0]["noise_param"])
    assert len(d.denoise([good], noise_param="auto")["out"]) == 1     # (and the model still runs)


# ---- 3. what the auto calls leave alone ------------------------------------------------------------------------------------------------------------
def test_auto_between_forward_backward_and_train_steps_changes_nothing():
    from test_hip_posterior import _batch, _denoiser
    from ssdn.params import PipelineOutput as PO
    data = [_batch("gauss25", 3, seed=k) for k in range(4)]
    noisy = _images(3, seed=2)[:1]

    def run(with_auto):
        d = _denoiser("gauss25", "known", 3)
        d.train()
        out = d.run_pipeline(data[3])
        if with_auto:
            d.denoise(noisy, noise_param="auto")
            d.estimate_noise(noisy)
        d.backward()
        kept = [out[PO.IMG_DENOISED].detach().clone(), out[PO.LOSS].detach().clone(), d.flat_grad.clone()]
        for k in range(2):
            d.train_step(data[k], lr=3e-4)
            if with_auto and k < 1:
                d.denoise(noisy, noise_param="auto", std=True)
        torch.cuda.synchronize()
        return kept + [d.flat.detach().clone(), d.adam_m.clone(), d.adam_v.clone()]
    a, b = run(False), run(True)
    assert all(torch.isfinite(t).all() for t in a) and float(a[2].abs().max()) > 0
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---- 4. the command, end to end ----------------------------------------------------------------------------------------------------------------------
def test_cli_denoise_auto_end_to_end(tmp_path):
    """a folder of three PNGs of different sizes through a 3-channel known-sigma model: the noise_param column is Denoiser.denoise's"""
    from PIL import Image
    from ssdn.__main__ import start_cli
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    images = _images(3, seed=3)
    for i, a in enumerate(images):
        Image.fromarray(a).save(imgs / ("im%d.png" % i))
    d = _model("gauss25", 3)
    torch.save({k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in d.state_dict().items()}, tmp_path / "model.wt")
    out_dir = tmp_path / "out"
    start_cli(["denoise", "-m", str(tmp_path / "model.wt"), "-i", str(imgs), "-o", str(out_dir), "--noise_param", "auto", "--batch_size", "2"])
    want = d.denoise(images, noise_param="auto", batch_size=2)
    with open(out_dir / "denoise.csv") as fh:
        rows = list(csv.DictReader(fh))
    assert [r["file"] for r in rows] == ["im0.png", "im1.png", "im2.png"]
    assert list(rows[0]) == ["file", "width", "height", "noise_std", "noise_param"]
    for i, r in enumerate(rows):
        assert float(np.float32(float(r["noise_param"]))) == want["noise_param"][i]
        assert np.array_equal(np.asarray(Image.open(out_dir / ("im%d.png" % i))), want["out"][i].numpy())
