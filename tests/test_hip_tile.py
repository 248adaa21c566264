"""GPU: SSDN_OP_TILE_IN / SSDN_OP_TILE_OUT (csrc/tile_io.hip) against the numpy model of tests/tile_ref.py bit for bit, and
`Denoiser.denoise(tile=...)` / `ssdn denoise --tile` against the host composition of the same plan's runs byte for byte, with what they
leave alone.

Nothing here has a tolerance except noise_std (a float64 mean of per-tile values the test forms itself: 1e-6 relative): the ops are exact
functions of their inputs, and a tiled `denoise` runs the same plan on the same input bits as the host composition."""
import csv
import os

import numpy as np
import pytest
import torch

import tile_ref as TR
from head_ops import DEV

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTE = 16, 0xAB


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. the ops against the model ------------------------------------------------------------------------------------------------------------
def tile_in_op(img, T, O, k0, B):
    """one SSDN_OP_TILE_IN launch -> dst [B,C,T,T] on the host; dst is NaN before the launch"""
    from ssdn.hip import engine as E
    h, w, Cn = img.shape
    src = torch.from_numpy(np.ascontiguousarray(img).reshape(-1)).to(DEV)
    dst = torch.full((B, Cn, T, T), float("nan"), dtype=torch.float32, device=DEV)
    E.tile_in(src, w, h, T, O, k0, dst)
    torch.cuda.synchronize()
    return dst.cpu().numpy()


def tile_out_op(store, w, h, T, O, mode, repeat=1):
    """`repeat` SSDN_OP_TILE_OUT launches into the middle of a buffer of guard bytes -> (the image part, the guards before and after it)"""
    from ssdn.hip import engine as E
    Cn = store.shape[1]
    nbytes = w * h * Cn * (4 if mode else 1)
    buf = torch.full((GUARD + nbytes + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
    dst = buf[GUARD:GUARD + nbytes]
    dst = dst.view(torch.float32) if mode else dst
    sd = torch.from_numpy(np.ascontiguousarray(store)).to(DEV)
    for _ in range(repeat):
        E.tile_out(sd, w, h, T, O, mode, dst)
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    body = out[GUARD:GUARD + nbytes]
    return (body.view(np.float32).reshape(Cn, h, w) if mode else body.reshape(h, w, Cn)), out[:GUARD], out[GUARD + nbytes:]


@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("T,O", TR.GPU_GRIDS)
def test_ops_against_the_numpy_model_bit_for_bit(T, O, Cn):
    for h, w in TR.GPU_SIZES:
        img = TR.make_image(h, w, Cn, seed=h + 3 * w + T)
        want = TR.tile_in_ref(img, T, O)
        n = want.shape[0]
        # TILE_IN: all tiles in batches of 3 (the last one short, k0 > 0 from the second on) and of 1
        for bs in (3, 1):
            for k0 in range(0, n, bs):
                B = min(bs, n - k0)
                got = tile_in_op(img, T, O, k0, B)
                assert not np.isnan(got).any()                               # every element was written
                assert np.array_equal(_bits(got), _bits(want[k0:k0 + B])), (h, w, k0, B)
        # TILE_OUT: a store of everything the blend and q must survive
        store = TR.make_store(n, Cn, T, seed=h + w + Cn)
        for mode in (0, 1):
            ref = TR.tile_out_ref(store, w, h, T, O, mode)
            got, before, after = tile_out_op(store, w, h, T, O, mode)
            assert (before == GUARD_BYTE).all() and (after == GUARD_BYTE).all()
            if mode == 0:
                assert np.array_equal(got, ref), (h, w, mode)
            else:
                nan = np.isnan(ref)
                assert np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(ref)[~nan]), (h, w, mode)
            again, _, _ = tile_out_op(store, w, h, T, O, mode, repeat=2)
            assert np.array_equal(again.view(np.uint8), got.view(np.uint8))


@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("T,O", TR.GPU_GRIDS)
def test_round_trip_on_the_device(T, O, Cn):
    from ssdn.hip import engine as E
    from ssdn.hip import lib as L
    for h, w in TR.GPU_SIZES:
        img = TR.make_image(h, w, Cn, seed=7 + h + w)
        n = L.tile_count(w, T, O) * L.tile_count(h, T, O)
        src = torch.from_numpy(img.reshape(-1)).to(DEV)
        store = torch.full((n, Cn, T, T), float("nan"), dtype=torch.float32, device=DEV)
        E.tile_in(src, w, h, T, O, 0, store)
        out = torch.zeros((h * w * Cn,), dtype=torch.uint8, device=DEV)
        E.tile_out(store, w, h, T, O, 0, out)
        assert torch.equal(out, src), (h, w)


# ---- 2. Denoiser.denoise(tile=...) against the host composition -------------------------------------------------------------------------------
# (name, algorithm, style, noise value, channels, noise_param of the call, its value in the metadata)
MODELS = [("ssdn_gauss_known", "ssdn", "gauss25", "known", 3, 25, 25 / 255),
          ("ssdn_poisson_var", "ssdn", "poisson30", "var", 1, None, None),
          ("n2c_plain", "n2c", "gauss25", None, 3, None, None)]
SIZES = [(70, 100), (40, 150), (24, 40)]                             # (h, w); the third fits one tile
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
        d.mark_dirty()
        _DEN[name] = d
    return _DEN[name]


def _images(ch, seed=0, sizes=SIZES):
    g = np.random.default_rng(300 + seed)
    return [g.integers(0, 256, size=(h, w, ch), dtype=np.uint8) for h, w in sizes]


def _host_composition(d, img, T, O, bs, npv, is_ssdn, poisson):
    """the tiles of the model, `bs` at a time through run_pipeline (the same inference plan and batch size), then the model's blend and q
    -> (bytes [h,w,C], std [C,h,w] or None, per-tile noise_std values or None)"""
    from ssdn.datasets import NoisyDataset
    from ssdn.params import PipelineOutput as PO
    h, w, Cn = img.shape
    tiles = TR.tile_in_ref(img, T, O)
    n, Kx, S = tiles.shape[0], TR.count(w, T, O), T - O
    store, store_std, nstd = np.zeros_like(tiles), np.zeros_like(tiles), []
    d.eval()
    for k0 in range(0, n, bs):
        B = min(bs, n - k0)
        data = [torch.from_numpy(tiles[k0:k0 + B]).to(DEV)]
        if npv is not None:
            data += [torch.zeros(0), {NoisyDataset.Metadata.INPUT_NOISE_VALUES: torch.full((B, 1, 1, 1), npv)}]
        with torch.no_grad():
            out = d.run_pipeline(data)
        store[k0:k0 + B] = out[PO.IMG_DENOISED].cpu().numpy()
        if is_ssdn:
            store_std[k0:k0 + B] = d.posterior(data)["std"].cpu().numpy()
            v = out[PO.NOISE_STD_DEV].cpu()
            for b in range(B):
                ky, kx = divmod(k0 + b, Kx)
                nstd.append(float(v[b, :min(T, w - kx * S), :min(T, h - ky * S)].double().mean()) if poisson else float(v.reshape(-1)[b]))
    return (TR.tile_out_ref(store, w, h, T, O, 0), TR.tile_out_ref(store_std, w, h, T, O, 1) if is_ssdn else None, nstd if is_ssdn else None)


@pytest.mark.parametrize("name,T,O", [(m[0], 64, 32) for m in MODELS] + [("ssdn_gauss_known", 96, None)])
def test_tiled_denoise_is_the_host_composition_byte_for_byte(name, T, O):
    _, alg, style, mode, ch, npar, npv = next(m for m in MODELS if m[0] == name)
    d = _model(name)
    is_ssdn = alg == "ssdn"
    images = _images(ch)
    d.train()                                                        # whatever the module's mode
    res = d.denoise(images, noise_param=npar, batch_size=2, std=is_ssdn, tile=T, overlap=O)
    assert d.training and d._last_train_engine is None
    assert set(res) == ({"out", "noise_std", "std", "tiles"} if is_ssdn else {"out", "tiles"})
    O = 32 if O is None else O                                       # (the default overlap of tile = 96)
    whole = d.denoise(images, noise_param=npar, batch_size=2, std=is_ssdn)
    for k, (h, w) in enumerate(SIZES):
        got = res["out"][k]
        assert got.dtype == torch.uint8 and tuple(got.shape) == (h, w, ch) and got.device.type == "cpu"
        n = TR.count(w, T, O) * TR.count(h, T, O)
        if w <= T and h <= T:                                        # the existing route, untouched
            assert res["tiles"][k] == 1 and torch.equal(got, whole["out"][k])
            if is_ssdn:
                assert torch.equal(res["std"][k], whole["std"][k]) and res["noise_std"][k] == whole["noise_std"][k]
            continue
        assert res["tiles"][k] == n and n > 1
        want, want_std, nstd = _host_composition(d, images[k], T, O, 2, npv, is_ssdn, style.startswith("poisson"))
        assert np.array_equal(got.numpy(), want), (name, k)
        assert len(np.unique(want)) > 8                              # (the network's output is an image, not a constant)
        if is_ssdn:
            assert tuple(res["std"][k].shape) == (ch, h, w) and np.array_equal(_bits(res["std"][k].numpy()), _bits(want_std))
            m = float(np.mean(np.asarray(nstd, dtype=np.float64)))
            assert abs(res["noise_std"][k] - m) <= 1e-6 * abs(m), (res["noise_std"][k], m)
    assert sum(1 for h, w in SIZES if w <= T and h <= T) == 1


def test_a_tile_that_holds_every_image_changes_nothing():
    d = _model("ssdn_gauss_known")
    images = _images(3, seed=1)
    a = d.denoise(images, noise_param=25, batch_size=2, std=True, uniform=True)
    b = d.denoise(images, noise_param=25, batch_size=2, std=True, uniform=True, tile=160, overlap=32)
    assert b.pop("tiles") == [1, 1, 1] and set(a) == set(b)
    for k in range(3):
        assert torch.equal(a["out"][k], b["out"][k]) and torch.equal(a["std"][k], b["std"][k]) and a["noise_std"][k] == b["noise_std"][k]
    gray = _model("ssdn_poisson_var").denoise([im[:, :, 0] for im in _images(1)[:1]], tile=64)     # [h, w] in, [h, w] out
    assert tuple(gray["out"][0].shape) == SIZES[0]


def test_auto_noise_parameter_is_the_whole_images_estimate():
    d = _model("ssdn_gauss_known")
    g = np.random.default_rng(5)
    # pictures with structure and noise, away from the clipped ends, so that the estimator has valid windows
    images = []
    for h, w in SIZES[:2]:
        yy, xx = np.mgrid[0:h, 0:w]
        clean = 128 + 60 * np.sin(xx / 9.0)[:, :, None] * np.cos(yy / 7.0)[:, :, None] + np.zeros((1, 1, 3))
        images.append(np.clip(clean + g.normal(0, 12, clean.shape), 1, 254).astype(np.uint8))
    res = d.denoise(images, noise_param="auto", batch_size=2, tile=64, overlap=32)
    est = d.estimate_noise(images)
    for k in range(2):
        p = res["noise_param"][k]
        assert np.isfinite(p) and np.float32(p).tobytes() == np.float32(est[k]["noise_param"]).tobytes()
        one = d.denoise([images[k]], noise_param=p, batch_size=2, tile=64, overlap=32)
        assert torch.equal(one["out"][0], res["out"][k])
    with pytest.raises(ValueError, match="image 0 has too few valid 3x3 windows"):
        d.denoise([np.zeros((70, 100, 3), dtype=np.uint8)], noise_param="auto", tile=64)


# ---- 3. what a tiled denoise leaves alone -----------------------------------------------------------------------------------------------------------
def test_tiled_denoise_between_forward_backward_and_train_steps_changes_nothing():
    from test_hip_posterior import _batch, _denoiser
    from ssdn.params import PipelineOutput as PO
    data = [_batch("gauss25", 3, seed=k) for k in range(4)]
    noisy = _images(3, seed=2)[:1]

    def run(with_denoise):
        d = _denoiser("gauss25", "known", 3)
        d.train()
        out = d.run_pipeline(data[3])
        if with_denoise:
            d.denoise(noisy, noise_param=25, tile=64, overlap=32, batch_size=2)
        d.backward()
        kept = [out[PO.IMG_DENOISED].detach().clone(), out[PO.LOSS].detach().clone(), d.flat_grad.clone()]
        for k in range(3):
            d.train_step(data[k], lr=3e-4)
            if with_denoise and k < 2:
                d.denoise(noisy, noise_param=25, std=True, tile=64, overlap=32, batch_size=2)
        torch.cuda.synchronize()
        return kept + [d.flat.detach().clone(), d.adam_m.clone(), d.adam_v.clone()]
    a, b = run(False), run(True)
    assert all(torch.isfinite(t).all() for t in a) and float(a[2].abs().max()) > 0
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---- 4. the command, end to end -------------------------------------------------------------------------------------------------------------------
def test_cli_denoise_tile_end_to_end(tmp_path):
    from PIL import Image
    from ssdn.__main__ import start_cli
    from ssdn.denoiser import Denoiser
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    images = _images(3, seed=4)
    for i, a in enumerate(images):
        Image.fromarray(a).save(imgs / ("im%d.png" % i))
    d = _model("ssdn_gauss_known")
    torch.save({k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in d.state_dict().items()}, tmp_path / "model.wt")
    out_dir = tmp_path / "out"
    start_cli(["denoise", "-m", str(tmp_path / "model.wt"), "-i", str(imgs), "-o", str(out_dir), "--noise_param", "25", "--batch_size", "2",
               "--std", "--tile", "64", "--overlap", "32"])
    want = Denoiser.from_state_dict(torch.load(tmp_path / "model.wt", map_location="cpu", weights_only=False)).denoise(
        images, noise_param=25, batch_size=2, std=True, tile=64, overlap=32)
    assert sorted(os.listdir(out_dir)) == sorted(["denoise.csv"] + ["im%d%s" % (i, s) for i in range(3) for s in (".png", "_std.npy")])
    for i, (h, w) in enumerate(SIZES):
        png = np.asarray(Image.open(out_dir / ("im%d.png" % i)))
        assert png.shape == (h, w, 3) and np.array_equal(png, want["out"][i].numpy())
        std = np.load(out_dir / ("im%d_std.npy" % i))
        assert std.dtype == np.float32 and std.shape == (3, h, w) and np.array_equal(std, want["std"][i].numpy())
    with open(out_dir / "denoise.csv") as fh:
        rows = list(csv.DictReader(fh))
    assert [r["file"] for r in rows] == ["im0.png", "im1.png", "im2.png"] and set(rows[0]) == {"file", "width", "height", "noise_std", "tiles"}
    assert [int(r["tiles"]) for r in rows] == want["tiles"] == [6, 4, 1]
    assert all(abs(float(r["noise_std"]) - want["noise_std"][i]) < 1e-6 for i, r in enumerate(rows))
