"""GPU: SSDN_OP_IMAGE_IN / SSDN_OP_IMAGE_OUT (csrc/image_io.hip) against the numpy model of tests/image_io_ref.py bit for bit, their guards
on inconsistent tables, `Denoiser.denoise` against the package's host route byte for byte, what it leaves alone, and `ssdn denoise`.

Nothing here has a tolerance except noise_std (a mean the test forms in another order than the method: 1e-6 relative): the ops are exact
functions of their inputs, and `denoise` runs the same plan on the same input bits as the host route."""
import csv
import os

import numpy as np
import pytest
import torch

import image_io_ref as IO
from head_ops import DEV, P, run_one

pytestmark = pytest.mark.gpu


# ---- 1. the ops against the model ------------------------------------------------------------------------------------------------------------
def image_in_op(buf, nbytes, offs, ext, Cn, H, W):
    """one SSDN_OP_IMAGE_IN launch on device copies -> dst [B,C,H,W] on the host; dst is NaN before the launch"""
    from ssdn.hip import lib as L
    B = len(offs)
    src = torch.from_numpy(np.ascontiguousarray(buf)).to(DEV)
    od = torch.tensor(offs, dtype=torch.int64, device=DEV)
    ed = torch.tensor(ext, dtype=torch.int32, device=DEV).contiguous()
    dst = torch.full((B, Cn, H, W), float("nan"), dtype=torch.float32, device=DEV)
    run_one("image_in", L.ImageInArgs(P(src), nbytes, P(od), P(ed), B, Cn, H, W, P(dst)))
    return dst.cpu().numpy()


def image_out_op(x, ext, offs, dst0, nbytes, repeat=1):
    """`repeat` SSDN_OP_IMAGE_OUT launches on device copies -> the byte buffer on the host; the buffer is dst0 before the first launch"""
    from ssdn.hip import lib as L
    B, Cn, H, W = x.shape
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    od = torch.tensor(offs, dtype=torch.int64, device=DEV)
    ed = torch.tensor(ext, dtype=torch.int32, device=DEV).contiguous()
    dst = torch.from_numpy(dst0.copy()).to(DEV)
    for _ in range(repeat):
        run_one("image_out", L.ImageOutArgs(P(xd), P(ed), P(od), P(dst), nbytes, B, Cn, H, W))
    return dst.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _planes(shape, seed):
    """an fp32 batch for IMAGE_OUT: values around [0, 1] and beyond, k/255 and its neighbours, and the special values"""
    g = np.random.default_rng(seed)
    x = g.uniform(-0.2, 1.2, shape).astype(np.float32)
    flat = x.reshape(-1)
    k = np.arange(256, dtype=np.float32) / np.float32(255.0)
    special = np.concatenate([k, np.nextafter(k, np.float32(2)), np.nextafter(k, np.float32(-1)),
                              np.array([-0.0, np.nan, np.inf, -np.inf, 1.0, -1e-30, 3e38], dtype=np.float32)])
    flat[g.choice(flat.size, special.size, replace=False)] = special
    return x


@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("H,W", IO.PADDED)
def test_ops_against_the_numpy_model_bit_for_bit(H, W, Cn):
    """six images of EXTENTS in one packed buffer with 16 guard bytes of 0xAB between them.  Inside 32 x 96 three of the extents exceed the
    tensor: the table says what the image is, both sides clamp it to the tensor"""
    ext = IO.EXTENTS
    images = IO.make_images(ext, Cn, seed=10 * H + Cn)
    buf, offs = IO.pack(images)
    got = image_in_op(buf, buf.size, offs, ext, Cn, H, W)
    assert not np.isnan(got).any()                                   # every element was written
    want = IO.image_in_ref(buf, buf.size, offs, ext, Cn, H, W)
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(image_in_op(buf, buf.size, offs, ext, Cn, H, W)), _bits(got))
    # out: into a buffer of guard bytes with a tail behind the last image
    x = _planes((len(ext), Cn, H, W), seed=H + Cn)
    dst0 = np.full(buf.size + 64, IO.GUARD_BYTE, dtype=np.uint8)
    out = image_out_op(x, ext, offs, dst0, dst0.size)
    assert np.array_equal(out, IO.image_out_ref(x, ext, offs, dst0.copy(), dst0.size))
    mask = np.ones(dst0.size, dtype=bool)
    for b, (e1, e2) in enumerate(ext):
        mask[offs[b]:offs[b] + min(e1, H) * min(e2, W) * Cn] = False
    assert (out[mask] == IO.GUARD_BYTE).all() and mask[-64:].all()
    assert np.array_equal(image_out_op(x, ext, offs, dst0, dst0.size, repeat=2), out)


@pytest.mark.parametrize("Cn", [1, 3])
def test_round_trip_on_the_device(Cn):
    ext = IO.fits(IO.EXTENTS, 64, 64)
    images = IO.make_images(ext, Cn, seed=3)
    buf, offs = IO.pack(images)
    x = image_in_op(buf, buf.size, offs, ext, Cn, 64, 64)
    out = image_out_op(x, ext, offs, np.full(buf.size, IO.GUARD_BYTE, dtype=np.uint8), buf.size)
    assert np.array_equal(out, buf)


def test_inconsistent_tables_are_clamped_and_guarded():
    """The buffers are what the arguments say; only the tables are wrong: extents beyond the tensor or negative, offsets that run past the
    byte count, start behind it or are negative, and a byte count below the buffer's size.  Reads outside give 0, writes outside are
    dropped, and the launch ends clean (the synchronize inside run_one raises otherwise)."""
    Cn, H, W = 3, 32, 64
    im = IO.make_images([(20, 30)], Cn, seed=5)[0]
    buf, offs = IO.pack([im] * 6)
    n = buf.size - 100                                               # the byte count the ops are told: the last image straddles it
    ext = [(20, 30), (999, 999), (-3, 30), (20, 30), (20, 30), (20, 30)]
    offs = [offs[0], offs[1], offs[2], n + 4096, -8, offs[5]]
    got = image_in_op(buf, n, offs, ext, Cn, H, W)
    want = IO.image_in_ref(buf, n, offs, ext, Cn, H, W)
    assert np.array_equal(_bits(got), _bits(want))
    assert (got[2] == 0).all() and (got[3] == 0).all() and (got[4] == 0).all() and (got[5] == 0).any() and (got[5] != 0).any()
    x = _planes((6, Cn, H, W), seed=9)
    dst0 = np.full(buf.size, IO.GUARD_BYTE, dtype=np.uint8)
    out = image_out_op(x, ext, offs, dst0, n)
    assert np.array_equal(out, IO.image_out_ref(x, ext, offs, dst0.copy(), n))
    # written: the clamped extents of samples 0, 1 (32 x 64: it runs over its neighbours, inside the buffer) and 5 (up to the byte count)
    mask = np.ones(buf.size, dtype=bool)
    for b in (0, 1, 5):
        mask[offs[b]:min(offs[b] + min(ext[b][0], H) * min(ext[b][1], W) * Cn, n)] = False
    assert (out[mask] == IO.GUARD_BYTE).all() and mask[n:].all() and mask[:16].all() and not mask[n - 1]
    torch.cuda.synchronize()


# ---- 2. Denoiser.denoise against the host route ------------------------------------------------------------------------------------------------
# (name, algorithm, style, noise value, channels, noise_param of the call, its value in the metadata)
MODELS = [("ssdn_gauss_known", "ssdn", "gauss25", "known", 3, 25, 25 / 255),
          ("ssdn_gauss_const", "ssdn", "gauss25", "const", 1, None, None),
          ("ssdn_poisson_var", "ssdn", "poisson30", "var", 3, None, None),
          ("ssdn_impulse_known", "ssdn", "impulse50", "known", 3, 50, 0.5),
          ("n2c_plain", "n2c", "gauss25", None, 3, None, None)]
SIZES = [(24, 40), (64, 64), (50, 33)]                               # (h, w)
_DEN = {}


def _model(name):
    """the model `name` with random weights (the constructor's He-normal draw under a fixed seed), built once and shared"""
    if name not in _DEN:
        import ssdn
        from ssdn.denoiser import Denoiser
        from ssdn.params import ConfigValue, NoiseAlgorithm, NoiseValue
        _, alg, style, mode, ch, _, _ = next(m for m in MODELS if m[0] == name)
        cfg = ssdn.cfg.base()
        cfg[ConfigValue.ALGORITHM] = NoiseAlgorithm(alg)
        cfg[ConfigValue.NOISE_STYLE] = style
        cfg[ConfigValue.IMAGE_CHANNELS] = ch
        if mode is not None:
            cfg[ConfigValue.NOISE_VALUE] = NoiseValue(mode)
        torch.manual_seed(11)
        d = Denoiser(ssdn.cfg.infer(cfg, model_only=True), device="cuda:0")
        if mode == "const":
            with torch.no_grad():
                d.l_params[Denoiser.ESTIMATED_SIGMA].fill_(1.7)
        d.mark_dirty()
        assert d.cfg[ConfigValue.BLINDSPOT] == (alg == "ssdn")
        _DEN[name] = d
    return _DEN[name]


def _images(ch, seed=0):
    g = np.random.default_rng(100 + seed)
    return [g.integers(0, 256, size=(h, w, ch), dtype=np.uint8) for h, w in SIZES]


def _padded_shapes(images, blind, uniform, bucket=32):
    """the rule of NoisyDataset.get_output_size on tensor axes (x, y): uniform, multiple, square"""
    up = lambda n: (n + bucket - 1) // bucket * bucket      # noqa: E731
    big = (max(im.shape[1] for im in images), max(im.shape[0] for im in images))
    res = []
    for im in images:
        H, W = (up(n) for n in (big if uniform else (im.shape[1], im.shape[0])))
        res.append((max(H, W),) * 2 if blind else (H, W))
    return res


@pytest.mark.parametrize("uniform", [True, False])
@pytest.mark.parametrize("name", [m[0] for m in MODELS])
def test_denoise_is_the_host_route_byte_for_byte(name, uniform):
    from ssdn.datasets import NoisyDataset
    from ssdn.params import ConfigValue, PipelineOutput as PO
    _, alg, style, mode, ch, npar, npv = next(m for m in MODELS if m[0] == name)
    d = _model(name)
    is_ssdn = alg == "ssdn"
    images = _images(ch)
    d.train()                                                        # whatever the module's mode
    res = d.denoise(images, noise_param=npar, batch_size=2, uniform=uniform, std=is_ssdn)
    assert d.training and d._last_train_engine is None
    assert set(res) == ({"out", "noise_std", "std"} if is_ssdn else {"out"})
    # the host route with the same batches: images of one padded shape, two at a time, in input order
    shapes = _padded_shapes(images, d.cfg[ConfigValue.BLINDSPOT], uniform)
    groups = {}
    for k, s in enumerate(shapes):
        groups.setdefault(s, []).append(k)
    assert len(groups) == (1 if uniform or is_ssdn else 2)
    d.eval()
    for (H, W), members in groups.items():
        for lo in range(0, len(members), 2):
            idx = members[lo:lo + 2]
            batch = [images[k] for k in idx]
            x = IO.host_in(batch, H, W).to(DEV)
            data = [x]
            if npv is not None:
                data += [torch.zeros(0), {NoisyDataset.Metadata.INPUT_NOISE_VALUES: torch.full((len(idx), 1, 1, 1), npv)}]
            with torch.no_grad():
                out = d.run_pipeline(data)
            want = IO.host_out(out[PO.IMG_DENOISED].cpu(), batch)
            post = d.posterior(data)["std"].cpu() if is_ssdn else None
            for b, k in enumerate(idx):
                h, w = SIZES[k]
                got = res["out"][k]
                assert got.dtype == torch.uint8 and tuple(got.shape) == (h, w, ch) and got.device.type == "cpu"
                assert np.array_equal(got.numpy(), want[b]), (name, uniform, k)
                assert len(np.unique(want[b])) > 8                   # (the network's output is an image, not a constant)
                if is_ssdn:
                    assert torch.equal(res["std"][k], post[b, :, :w, :h].permute(0, 2, 1)) and tuple(res["std"][k].shape) == (ch, h, w)
                    nstd = out[PO.NOISE_STD_DEV].cpu().double()
                    nstd = nstd[b, :w, :h].mean() if style.startswith("poisson") else nstd.reshape(-1)[0 if mode == "const" else b]
                    assert abs(res["noise_std"][k] - float(nstd)) <= 1e-6 * abs(float(nstd)), (res["noise_std"][k], float(nstd))


def test_denoise_takes_tensors_gray_arrays_and_buckets():
    d = _model("ssdn_gauss_const")
    images = _images(1, seed=1)
    a = d.denoise(images, batch_size=3, uniform=True)
    b = d.denoise([torch.from_numpy(im[:, :, 0]) for im in images], batch_size=3, bucket=64)      # [h, w] tensors; 64 pads all three alike
    for x, y, (h, w) in zip(a["out"], b["out"], SIZES):
        assert tuple(y.shape) == (h, w) and torch.equal(x[:, :, 0], y)
    with pytest.raises(ValueError, match="bucket must be a positive multiple of 32"):
        d.denoise(images, bucket=48)


# ---- 3. what denoise leaves alone ---------------------------------------------------------------------------------------------------------------
def test_denoise_between_forward_backward_and_train_steps_changes_nothing():
    from test_hip_posterior import _batch, _denoiser
    from ssdn.params import PipelineOutput as PO
    data = [_batch("gauss25", 3, seed=k) for k in range(4)]
    noisy = _images(3, seed=2)[:1]

    def run(with_denoise):
        d = _denoiser("gauss25", "known", 3)
        d.train()
        out = d.run_pipeline(data[3])
        if with_denoise:
            d.denoise(noisy, noise_param=25)
        d.backward()
        kept = [out[PO.IMG_DENOISED].detach().clone(), out[PO.LOSS].detach().clone(), d.flat_grad.clone()]
        for k in range(3):
            d.train_step(data[k], lr=3e-4)
            if with_denoise and k < 2:
                d.denoise(noisy, noise_param=25, std=True)
        torch.cuda.synchronize()
        return kept + [d.flat.detach().clone(), d.adam_m.clone(), d.adam_v.clone()]
    a, b = run(False), run(True)
    assert all(torch.isfinite(t).all() for t in a) and float(a[2].abs().max()) > 0
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---- 4. the command, end to end -------------------------------------------------------------------------------------------------------------------
def test_cli_denoise_end_to_end(tmp_path):
    """a folder of three PNGs of different sizes, one of them grayscale, through a 3-channel known-sigma model, with --std"""
    from PIL import Image
    from ssdn.__main__ import start_cli
    from ssdn.denoiser import Denoiser
    from ssdn.utils.data import set_color_channels
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    g = np.random.default_rng(21)
    sizes = [(24, 40), (33, 50), (32, 32)]                           # (h, w)
    for i, (h, w) in enumerate(sizes):
        a = g.integers(0, 256, size=(h, w) if i == 1 else (h, w, 3), dtype=np.uint8)
        Image.fromarray(a).save(imgs / ("im%d.png" % i))
    d = _model("ssdn_gauss_known")
    torch.save({k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in d.state_dict().items()}, tmp_path / "model.wt")
    out_dir = tmp_path / "out"
    start_cli(["denoise", "-m", str(tmp_path / "model.wt"), "-i", str(imgs), "-o", str(out_dir), "--noise_param", "25", "--batch_size", "2",
               "--std"])
    loaded = [np.asarray(set_color_channels(Image.open(imgs / ("im%d.png" % i)), 3)) for i in range(3)]
    assert all(a.shape == (h, w, 3) for a, (h, w) in zip(loaded, sizes))
    want = Denoiser.from_state_dict(torch.load(tmp_path / "model.wt", map_location="cpu", weights_only=False)).denoise(
        loaded, noise_param=25, batch_size=2, std=True)
    assert sorted(os.listdir(out_dir)) == sorted(["denoise.csv"] + ["im%d%s" % (i, s) for i in range(3) for s in (".png", "_std.npy")])
    for i, (h, w) in enumerate(sizes):
        png = np.asarray(Image.open(out_dir / ("im%d.png" % i)))
        assert png.shape == (h, w, 3) and np.array_equal(png, want["out"][i].numpy())
        std = np.load(out_dir / ("im%d_std.npy" % i))
        assert std.dtype == np.float32 and std.shape == (3, h, w) and np.array_equal(std, want["std"][i].numpy())
    with open(out_dir / "denoise.csv") as fh:
        rows = list(csv.DictReader(fh))
    assert [r["file"] for r in rows] == ["im0.png", "im1.png", "im2.png"] and set(rows[0]) == {"file", "width", "height", "noise_std"}
    assert [(int(r["height"]), int(r["width"])) for r in rows] == sizes
    assert all(abs(float(r["noise_std"]) - want["noise_std"][i]) < 1e-6 for i, r in enumerate(rows))
