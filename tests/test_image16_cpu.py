"""No GPU: the 16-bit sample model (tests/image16_ref.py) -- its round trip, clamp and quantiser edges, its equivalence to the byte ops'
models at white = 255 --, the C ABI of the five 16-bit ops and their host-side refusals, `load_image` / `save_image16`, the refusals of
`Denoiser.denoise` and `estimate_noise` that come before any device work, the 16-bit `ImagePool` (from files and from arrays) with the
stream's torch path, and the trainer's `white`."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import image16_ref as R
import image_io_ref as IO
import patch_pool_ref as PP
import tile_ref as TR
import ssdn
from ssdn.datasets import DevicePoolStream, ImagePool, NoisyDataset, UnlabelledImageFolderDataset
from ssdn.hip import lib as L
from ssdn.params import ConfigValue, NoiseAlgorithm, NoiseValue, PipelineOutput

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MD = NoisyDataset.Metadata
OPS = ["image_in16", "image_out16", "tile_in16", "tile_out16", "pool_patch16"]
F32 = np.float32


# ---- 1. the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_struct_size():
    hdr = open(os.path.join(ROOT, "include", "ssdn_hip.h")).read()
    lib = L.load()
    for num, op in enumerate(OPS, 35):
        assert re.search(r"SSDN_OP_%s\s*=\s*%d\b" % (op.upper(), num), hdr) and L.OP[op] == num
        assert "} ssdn_%s_args;" % op in hdr
        assert lib.ssdn_struct_size(num) == C.sizeof(L.ARG_TYPES[op]) > 0
    assert re.search(r"#define SSDN_ABI_VERSION 19\b", hdr) and L.ABI_VERSION == 19 and lib.ssdn_abi_version() == 19
    assert [n for n, _ in L.ImageIn16Args._fields_] == ["src", "src_count", "offs", "ext", "B", "C", "H", "W", "white", "dst"]
    assert [n for n, _ in L.ImageOut16Args._fields_] == ["x", "ext", "offs", "dst", "dst_count", "B", "C", "H", "W", "white"]
    assert [n for n, _ in L.TileOut16Args._fields_] == ["store", "w", "h", "C", "T", "O", "Kx", "Ky", "white", "dst", "dst_count"]
    # the byte ops' structs are what they were
    assert lib.ssdn_struct_size(29) == 56 and lib.ssdn_struct_size(30) == 56 and lib.ssdn_struct_size(34) == C.sizeof(L.PoolPatchArgs)


_DUMMY = dict(
    image_in16=dict(src=0x1000, src_count=64, offs=0x1000, ext=0x1000, B=1, C=3, H=32, W=32, white=65535, dst=0x1000),
    image_out16=dict(x=0x1000, ext=0x1000, offs=0x1000, dst=0x1000, dst_count=64, B=1, C=3, H=32, W=32, white=65535),
    tile_in16=dict(src=0x1000, src_count=64 * 64, w=64, h=64, C=1, T=64, O=0, Kx=1, Ky=1, k0=0, B=1, white=65535, dst=0x1000),
    tile_out16=dict(store=0x1000, w=64, h=64, C=1, T=64, O=0, Kx=1, Ky=1, white=65535, dst=0x1000, dst_count=64 * 64),
    pool_patch16=dict(pool=0x1000, offsets=0x1000, sizes=0x1000, index=0x1000, noisy32=0x1000, N=1, B=1, C=1, P=8, white=65535))


def _refused(op, **kw):
    """run one op with dummy (never dereferenced) pointers -> the library's error text"""
    f = dict(_DUMMY[op])
    f.update(kw)
    a = L.ARG_TYPES[op](**f)
    rec = (L.OpRec * 1)()
    rec[0].type, rec[0].lane, rec[0].args = L.OP[op], 0, C.cast(C.pointer(a), C.c_void_p)
    lib = L.load()
    assert lib.ssdn_run_ops(rec, 1, None) != 0
    return lib.ssdn_last_error().decode()


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("white", [0, -1, 65536])
def test_white_outside_its_range_is_refused_without_a_gpu(op, white):
    err = _refused(op, white=white)
    assert re.search(r"^op 0 \(type %d\): %s: white must lie in \[1, 65535\]" % (L.OP[op], op), err), err


@pytest.mark.parametrize("op,kw,msg", [
    ("image_in16", dict(src=None), "must be given"), ("image_in16", dict(C=2), "C must be 1 or 3"),
    ("image_in16", dict(src_count=-1), "count must not be negative"), ("image_in16", dict(B=65536), "at most 65535"),
    ("image_out16", dict(x=None), "must be given"), ("image_out16", dict(H=0), "B, H and W must be at least 1"),
    ("image_out16", dict(dst_count=-1), "count must not be negative"),
    ("tile_in16", dict(T=48), "T must be a positive multiple of 32"), ("tile_in16", dict(O=64), "0 <= 2 O <= T"),
    ("tile_in16", dict(Kx=2), "the grid must be Kx = 1, Ky = 1"), ("tile_in16", dict(k0=1), "must lie inside the grid"),
    ("tile_in16", dict(src_count=64 * 64 - 1), "src_count is below w h C"), ("tile_in16", dict(C=2), "C must be 1 or 3"),
    ("tile_in16", dict(w=1 << 16, h=1 << 15, Kx=1024, Ky=512), "w h C must be below 2\\^31"),
    ("tile_out16", dict(dst=None), "must be given"), ("tile_out16", dict(dst_count=64 * 64 - 1), "dst_count is below"),
    ("pool_patch16", dict(pool=None), "are required"), ("pool_patch16", dict(P=0), "empty shape"),
    ("pool_patch16", dict(param_out=0x1000), "param_out needs the params table"),
    ("pool_patch16", dict(n2v_box=8, n2v_radius=2), "needs a coords output"),
    ("pool_patch16", dict(n2v_box=3, n2v_radius=2, coords=0x1000), "multiple of n2v_box"),
    ("pool_patch16", dict(B=1 << 20, C=3, P=1024), "32-bit indexing")])
def test_the_siblings_refusals_under_the_new_prefixes(op, kw, msg):
    err = _refused(op, **kw)
    assert re.search(r"^op 0 \(type %d\): %s: .*%s" % (L.OP[op], op, msg), err), err


def test_planned_lists_know_nothing_of_the_ops():
    for f in (("selfsupervised-denoising_amd", "ssdn", "hip", "graph.py"), ("oracle", "interp.py")):
        text = open(os.path.join(ROOT, *f)).read().lower()
        assert "in16" not in text and "patch16" not in text


# ---- 2. the sample model --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("white", [1, 3, 255, 1000, 4095, 50000, 65535])
def test_round_trip_of_every_sample(white):
    s = np.arange(white + 1, dtype=np.uint16)
    v = R.sample_in(s, white)
    assert v.dtype == np.float32 and v[0] == 0 and v[-1] == 1 and np.all(np.diff(v) > 0)
    assert np.array_equal(R.q16(v, white), s)


def test_truncation_would_fail_the_round_trip():
    """why q16 rounds where the byte ops' q truncates: the counts the definition quotes"""
    for white, bad in ((1000, 5), (50000, 2667)):
        s = np.arange(white + 1, dtype=np.uint16)
        assert int((R.q16_truncating(R.sample_in(s, white), white) != s).sum()) == bad


@pytest.mark.parametrize("white", [1, 255, 4095, 50000])
def test_samples_above_white_are_exactly_one(white):
    s = np.array([white, white + 1, min(2 * white, 65535), 65535], dtype=np.uint16)
    assert np.array_equal(R.sample_in(s, white), np.ones(4, dtype=np.float32))
    assert np.array_equal(R.q16(R.sample_in(s, white), white), np.full(4, white, dtype=np.uint16))


@pytest.mark.parametrize("white", [3, 255, 4095, 65535])
def test_quantiser_on_its_edges(white):
    k = np.unique(np.concatenate([np.arange(0, min(white, 300) + 1), np.arange(max(white - 300, 0), white + 1)]))
    v = (k.astype(F32) / F32(white)).astype(F32)
    for cand in (v, np.nextafter(v, F32(2)), np.nextafter(v, F32(-1))):
        # the model against exact arithmetic: the float32 product in float64, rounded to nearest even
        c = np.clip(cand.astype(np.float64), 0, 1)
        prod = (c.astype(F32) * F32(white)).astype(F32).astype(np.float64)
        assert np.array_equal(R.q16(cand, white), np.rint(prod).astype(np.uint16))
    assert np.array_equal(R.q16(v, white), k.astype(np.uint16))
    # exact .5 ties go to the even neighbour: (k + 0.5) / white is a tie only where the product lands on k + 0.5, so build the ties directly
    # with a power-of-two white, where the product is exact
    ties = (np.arange(0, 64).astype(F32) + F32(0.5)) / F32(1024)
    got = R.q16(ties, 1024)
    assert np.array_equal(got, np.array([k if k % 2 == 0 else k + 1 for k in range(64)], dtype=np.uint16))
    special = np.array([-0.0, np.nan, np.inf, -np.inf, 3e38, -3e38, 1.0, np.nextafter(F32(1), F32(0)), 1e-30], dtype=F32)
    want = [0, 0, white, 0, white, 0, white, int(np.rint(np.float64(np.nextafter(F32(1), F32(0)) * F32(white)))), 0]
    assert R.q16(special, white).tolist() == want


@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("H,W", IO.PADDED)
def test_in_models_at_white_255_are_the_byte_models(H, W, Cn):
    ext = IO.fits(IO.EXTENTS, H, W)
    images = IO.make_images(ext, Cn, seed=H + Cn)
    buf, offs = IO.pack(images)
    want = IO.image_in_ref(buf, buf.size, offs, ext, Cn, H, W)
    got = R.image_in16_ref(R.widen(buf), buf.size, offs, ext, Cn, H, W, 255)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("T,O", TR.GPU_GRIDS)
def test_tile_in_model_at_white_255_is_the_byte_model(T, O):
    img = TR.make_image(70, 100, 3, seed=T)
    assert np.array_equal(R.tile_in16_ref(R.widen(img), T, O, 255).view(np.uint32), TR.tile_in_ref(img, T, O).view(np.uint32))
    store = TR.make_store(TR.count(100, T, O) * TR.count(70, T, O), 3, T, seed=O)
    # and out: q16 at white 255 differs from q only by its rounding
    a, b = R.tile_out16_ref(store, 100, 70, T, O, 255), TR.tile_out_ref(store, 100, 70, T, O, 0)
    assert a.dtype == np.uint16 and a.shape == b.shape and np.all((a.astype(int) - b.astype(int) >= 0) & (a.astype(int) - b.astype(int) <= 1))


@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("box", [0, 8])
def test_pool_model_at_white_255_is_the_byte_model(Cn, box):
    imgs = PP.case_images(Cn)
    kw = dict(params=np.arange(7) * 0.01, n2v_box=box)
    want = PP.pool_patch_model(imgs, PP.INDEXES[1], 8, True, PP.SEED, PP.OFFSETS[0], **kw)
    got = R.pool_patch16_model([R.widen(im) for im in imgs], PP.INDEXES[1], 8, True, PP.SEED, PP.OFFSETS[0], 255, **kw)
    for k in ("noisy", "ref", "param"):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
    assert np.array_equal(got["origin"], want["origin"])
    assert box == 0 or np.array_equal(got["coords"], want["coords"])


def test_inconsistent_tables_in_the_model():
    """extents beyond the tensor and negative, offsets past the count, behind it and negative, a count below the buffer"""
    Cn, H, W, white = 3, 32, 64, 4095
    images = R.make_images16([(8, 8)] * 6, Cn, 5, white)
    buf, offs = R.pack_samples(images)
    ext = [(40, 70), (-3, 8), (8, 8), (8, 8), (8, 8), (8, 8)]
    offs = [offs[0], offs[1], buf.size + 5, buf.size - 10, -4, offs[5]]
    count = buf.size - 100
    got = R.image_in16_ref(buf, count, offs, ext, Cn, H, W, white)
    assert not got[1].any() and not got[2].any() and not got[3].any() and not got[4].any() and got[0].any()
    dst = np.full(buf.size, R.GUARD_SAMPLE, dtype=np.uint16)
    R.image_out16_ref(np.full((6, Cn, H, W), 0.5, dtype=F32), ext, offs, dst, count, white)
    changed = np.flatnonzero(dst != R.GUARD_SAMPLE)
    assert changed.size and changed.max() < count and not dst[count:].tolist().count(2048)


# ---- 3. files -------------------------------------------------------------------------------------------------------------------------------
def _ramp16(h=7, w=9, seed=0):
    a = np.random.default_rng(seed).integers(0, 65536, size=(h, w)).astype(np.uint16)
    a.reshape(-1)[:3] = (0, 65535, 256)
    return a


@pytest.mark.parametrize("ext", ["png", "tif"])
def test_16_bit_files_read_back_exactly(tmp_path, ext):
    from PIL import Image
    from ssdn.utils import load_image, save_image16
    a = _ramp16()
    Image.fromarray(a).save(str(tmp_path / ("a." + ext)))
    got = load_image(str(tmp_path / ("a." + ext)), 1)
    assert got.dtype == np.uint16 and got.shape == (7, 9, 1) and np.array_equal(got[:, :, 0], a)
    for arr in (a, a[:, :, None], torch.from_numpy(a.copy())):
        save_image16(arr, str(tmp_path / ("b." + ext)))
        with Image.open(str(tmp_path / ("b." + ext))) as im:
            assert im.mode.startswith("I;16")
        assert np.array_equal(load_image(str(tmp_path / ("b." + ext)), 1)[:, :, 0], a)
    with pytest.raises(ValueError, match="16-bit files are single-channel: use a model trained with --mono"):
        load_image(str(tmp_path / ("a." + ext)), 3)
    with pytest.raises(ValueError, match="uint16"):
        save_image16(a.astype(np.uint8), str(tmp_path / "c.png"))


def test_8_bit_files_take_the_old_route_and_mode_I_is_checked(tmp_path):
    from PIL import Image
    from ssdn.utils import load_image, set_color_channels
    rgb = np.random.default_rng(1).integers(0, 256, size=(5, 6, 3)).astype(np.uint8)
    Image.fromarray(rgb).save(str(tmp_path / "rgb.png"))
    Image.fromarray(rgb[:, :, 0]).save(str(tmp_path / "grey.png"))
    for name in ("rgb.png", "grey.png"):
        for ch in (1, 3):
            with Image.open(str(tmp_path / name)) as im:
                want = np.asarray(set_color_channels(im, ch), dtype=np.uint8)
            got = load_image(str(tmp_path / name), ch)
            assert got.dtype == np.uint8 and got.shape == (5, 6, ch) and np.array_equal(got.reshape(want.shape), want)
    ok = np.array([[0, 65535], [300, 7]], dtype=np.int32)
    Image.fromarray(ok, mode="I").save(str(tmp_path / "i_ok.tif"))
    got = load_image(str(tmp_path / "i_ok.tif"), 1)
    assert got.dtype == np.uint16 and np.array_equal(got[:, :, 0], ok)
    bad = ok.copy()
    bad[1, 1] = 70000
    Image.fromarray(bad, mode="I").save(str(tmp_path / "i_bad.tif"))
    with pytest.raises(ValueError, match="i_bad.tif"):
        load_image(str(tmp_path / "i_bad.tif"), 1)


# ---- 4. Denoiser.denoise and estimate_noise: refusals before any device work ---------------------------------------------------------------------
def _cpu_denoiser(algorithm, style, value=None, channels=1):
    from ssdn.denoiser import Denoiser
    cfg = ssdn.cfg.base()
    cfg[ConfigValue.ALGORITHM] = algorithm
    cfg[ConfigValue.NOISE_STYLE] = style
    cfg[ConfigValue.IMAGE_CHANNELS] = channels
    if value is not None:
        cfg[ConfigValue.NOISE_VALUE] = value
    return Denoiser(ssdn.cfg.infer(cfg, model_only=True), device="cpu")


def test_denoise_refusals_need_no_device():
    known = _cpu_denoiser(NoiseAlgorithm.SELFSUPERVISED_DENOISING, "gauss25", NoiseValue.KNOWN)
    g16, g8 = np.zeros((8, 9), dtype=np.uint16), np.zeros((8, 9), dtype=np.uint8)
    with pytest.raises(ValueError, match="estimator is defined on bytes.*pass the noise parameter as a number"):
        known.denoise([g8, g16], noise_param="auto")
    with pytest.raises(ValueError, match="estimator is defined on bytes.*pass the noise parameter as a number"):
        known.estimate_noise([g16])
    with pytest.raises(ValueError, match="white is the white level of uint16 images and this call has none"):
        known.denoise([g8], noise_param=25, white=4095)
    with pytest.raises(ValueError, match="white is the white level of uint16 images and this call has none"):
        known.denoise([], noise_param=25, white=4095)
    for bad in (0, 65536, -5, 1.5):
        with pytest.raises(ValueError, match=r"white must be an integer in \[1, 65535\]"):
            known.denoise([g16], noise_param=25, white=bad)
    with pytest.raises(ValueError, match="uint8"):
        known.denoise([g16.astype(np.float32)], noise_param=25)
    with pytest.raises(ValueError, match="has 3 channel"):
        known.denoise([np.zeros((8, 9, 3), dtype=np.uint16)], noise_param=25)
    assert known.denoise([], noise_param=25) == {"out": [], "noise_std": []}


def test_cli_denoise_white_flag():
    from ssdn.cli.cli import build_parser
    parser, _ = build_parser()
    a = vars(parser.parse_args(["denoise", "-m", "x.wt", "-i", "imgs", "-o", "out"]))
    b = vars(parser.parse_args(["denoise", "-m", "x.wt", "-i", "imgs", "-o", "out", "--white", "4095"]))
    assert a["white"] is None and b["white"] == 4095


# ---- 5. the pool ----------------------------------------------------------------------------------------------------------------------------
SIZES16 = ((5, 9), (12, 4), (8, 8), (3, 40))


def _folder16(tmp_path):
    from PIL import Image
    arrays = [_ramp16(h, w, seed=k) for k, (h, w) in enumerate(SIZES16)]
    for k, a in enumerate(arrays):
        Image.fromarray(a).save(str(tmp_path / ("im%d.png" % k)))
    return arrays


def test_pool_of_a_16_bit_folder(tmp_path):
    from PIL import Image
    arrays = _folder16(tmp_path)
    ds = UnlabelledImageFolderDataset(str(tmp_path), channels=1)
    pool = ImagePool(ds, "cpu")
    samples = sum(a.size for a in arrays)
    assert pool.bits == 16 and pool.white == 65535 and pool.pool.dtype == torch.uint16 and pool.channels == 1
    assert pool.nbytes == 2 * samples and pool.pool.numel() == samples
    assert pool.sizes_host.tolist() == [[w, h] for h, w in SIZES16]                      # rows run along the picture's x
    assert pool.offsets_host.tolist() == np.cumsum([0] + [a.size for a in arrays])[:-1].tolist()      # in samples
    for k, a in enumerate(arrays):
        assert pool.image(k).dtype == torch.uint16 and np.array_equal(pool.image(k).numpy()[0], a.T)
        assert np.array_equal(pool.upright(k).numpy()[:, :, 0], a)
    assert ImagePool(ds, "cpu", white=4095).white == 4095
    assert ImagePool(ds, "cpu", max_bytes=2 * samples).nbytes == 2 * samples
    with pytest.raises(ValueError) as e:
        ImagePool(ds, "cpu", max_bytes=2 * samples - 1)
    assert str(2 * samples) in str(e.value) and str(2 * samples - 1) in str(e.value)
    for bad in (0, 65536):
        with pytest.raises(ValueError, match=r"white must be an integer in \[1, 65535\]"):
            ImagePool(ds, "cpu", white=bad)
    with pytest.raises(ValueError, match="estimator is defined on bytes"):
        pool.estimate_params(None, "gauss")
    with pytest.raises(ValueError, match="use a model trained with --mono"):
        ImagePool(UnlabelledImageFolderDataset(str(tmp_path), channels=3), "cpu")
    # one 8-bit file among them: refused, naming a file of each depth
    Image.fromarray(arrays[0].astype(np.uint8)).save(str(tmp_path / "im9.png"))
    with pytest.raises(ValueError) as e:
        ImagePool(UnlabelledImageFolderDataset(str(tmp_path), channels=1), "cpu")
    assert "im9.png" in str(e.value) and "im0.png" in str(e.value)


def test_8_bit_pools_are_what_they_were(tmp_path):
    from PIL import Image
    rs = np.random.RandomState(3)
    arrays = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((5, 9), (12, 4))]
    for k, a in enumerate(arrays):
        Image.fromarray(a).save(str(tmp_path / ("im%d.png" % k)))
    ds = UnlabelledImageFolderDataset(str(tmp_path), channels=3)
    pool, made = ImagePool(ds, "cpu"), ImagePool.from_images(arrays, "cpu")
    for p in (pool, made):
        assert p.bits == 8 and p.white is None and p.pool.dtype == torch.uint8 and p.nbytes == sum(a.size for a in arrays)
    assert torch.equal(pool.pool, made.pool) and torch.equal(pool.offsets_host, made.offsets_host) and torch.equal(pool.sizes_host, made.sizes_host)
    assert made.channels == 3 and made.n == 2 and made.files is None
    for p in (lambda: ImagePool(ds, "cpu", white=255), lambda: ImagePool.from_images(arrays, "cpu", white=255)):
        with pytest.raises(ValueError, match="white is the white level of a 16-bit pool"):
            p()
    with pytest.raises(ValueError, match="uint8 and uint16 images in one pool"):
        ImagePool.from_images([arrays[0], arrays[1].astype(np.uint16)], "cpu")
    with pytest.raises(ValueError, match="cap"):
        ImagePool.from_images(arrays, "cpu", max_bytes=10)
    with pytest.raises(ValueError, match="not a uint8 or uint16"):
        ImagePool.from_images([arrays[0].astype(np.float32)], "cpu")


ALGOS = {"ssdn": NoiseAlgorithm.SELFSUPERVISED_DENOISING, "n2v": NoiseAlgorithm.NOISE_TO_VOID}


@pytest.mark.parametrize("algo", ["ssdn", "n2v"])
@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("white", [65535, 4095])
def test_cpu_stream_of_a_16_bit_pool(algo, Cn, white):
    upright = R.make_images16([(c, r) for r, c in PP.SIZES], Cn, 7, white)               # [h, w, C]
    pool = ImagePool.from_images(upright, "cpu", white=None if white == 65535 else white)
    assert pool.bits == 16 and pool.white == white and pool.channels == Cn
    planar = [im.transpose(2, 1, 0) for im in upright]                                   # [C, rows = w, cols = h]
    for i, im in enumerate(planar):
        assert np.array_equal(pool.image(i).numpy(), im)
    st = DevicePoolStream(pool, [list(b) for b in PP.INDEXES[:2]], ALGOS[algo], "gauss25", 8, seed=11, augment=True)
    st.keep_origin = True
    for idx, (inp, ref, meta) in zip(PP.INDEXES[:2], st):
        plain = np.stack([R.sample_in(PP.cut(planar[i], 8, *[int(v) for v in st.last_origin[b]]), white) for b, i in enumerate(idx)])
        assert inp.dtype == torch.float32 and inp.shape == (5, Cn, 8, 8) and plain.max() <= 1.0
        assert white == 65535 or (plain == 1.0).any()                   # samples above white are in the patches, clamped
        if algo == "ssdn":
            assert np.array_equal(inp.numpy().view(np.uint32), plain.view(np.uint32))
        else:
            assert np.array_equal(ref.numpy().view(np.uint32), plain.view(np.uint32))
            co = meta[MD.MASK_COORDS]
            changed = {tuple(t) for t in np.argwhere((inp.numpy() != plain).any(1))}
            assert changed <= {(b, int(co[b, 0, 1]), int(co[b, 0, 0])) for b in range(5)}


# ---- 6. the trainer -------------------------------------------------------------------------------------------------------------------------
def _cfg(algo="ssdn", style="gauss25", value="known", patch=32):
    cfg = ssdn.cfg.base()
    cfg[ConfigValue.ALGORITHM] = NoiseAlgorithm(algo)
    cfg[ConfigValue.NOISE_STYLE] = style
    cfg[ConfigValue.NOISE_VALUE] = NoiseValue(value)
    cfg[ConfigValue.TRAIN_PATCH_SIZE] = patch
    cfg[ConfigValue.IMAGE_CHANNELS] = 1
    return cfg


def test_check_noisy_and_white():
    from ssdn.train import check_noisy
    with pytest.raises(ValueError, match="--white .* needs --noisy"):
        check_noisy(_cfg(), None, white=4095)
    for bad in (0, 65536, -1):
        with pytest.raises(ValueError, match=r"--white must be an integer in \[1, 65535\]"):
            check_noisy(_cfg(), "style", white=bad)
    check_noisy(_cfg(), "style", white=4095)
    check_noisy(_cfg(), "style", white=1)
    check_noisy(_cfg(), "auto", white=65535)          # (the depth is known only when the pool is built: refused there)


def test_cli_train_white_goes_through_the_parser(capsys, tmp_path):
    from ssdn.__main__ import start_cli
    from ssdn.cli.cli import build_parser
    base = ["train", "start", "-t", str(tmp_path), "-i", "8", "--algorithm", "ssdn", "--noise_value", "known", "--noise_style", "gauss25",
            "--mono", "--runs_dir", str(tmp_path / "runs")]
    parser, _ = build_parser()
    assert vars(parser.parse_args(base))["white"] is None and vars(parser.parse_args(base + ["--noisy", "--white", "4095"]))["white"] == 4095
    for extra, text in ((["--white", "4095"], "needs --noisy"), (["--noisy", "--white", "0"], "must be an integer in")):
        with pytest.raises(SystemExit):
            start_cli(base + extra)
        assert text in capsys.readouterr().err
    assert not os.path.exists(tmp_path / "runs")


def _stub(cfg):
    from ssdn.denoiser import Denoiser

    class Stub(Denoiser):
        def __init__(self, cfg):
            super().__init__(cfg, device="cpu")
            self.batches = []

        def train_step(self, data, lr, exchange=None):
            inp, meta = data[NoisyDataset.INPUT], data[NoisyDataset.METADATA]
            self.batches.append((meta[MD.INDEXES].tolist(), inp.clone()))
            n = inp.shape[0]
            return {PipelineOutput.INPUTS: data, PipelineOutput.LOSS: torch.ones(n, 1), PipelineOutput.IMG_DENOISED: inp.clone(),
                    PipelineOutput.IMG_MU: inp.clone(), PipelineOutput.NOISE_STD_DEV: torch.ones(n, 1, 1),
                    PipelineOutput.MODEL_STD_DEV: torch.ones(n, inp.shape[2], inp.shape[3])}
    return Stub(cfg)


def _train(tmp_path, folder, runs, noisy="style", white=None, iters=8):
    from ssdn.train import DenoiserTrainer
    cfg = _cfg()
    cfg[ConfigValue.TRAIN_ITERATIONS], cfg[ConfigValue.TRAIN_MINIBATCH_SIZE] = iters, 4
    cfg[ConfigValue.TRAIN_DATA_PATH], cfg[ConfigValue.DATALOADER_WORKERS] = folder, 0
    cfg[ConfigValue.PRINT_INTERVAL], cfg[ConfigValue.EVAL_INTERVAL], cfg[ConfigValue.SNAPSHOT_INTERVAL] = 4, 10 ** 9, 4
    torch.manual_seed(3)
    tr = DenoiserTrainer(cfg, runs_dir=str(tmp_path / runs))
    tr.noisy, tr.white = noisy, white
    tr.device_data = False
    tr.denoiser = _stub(tr.cfg)
    tr.init_state()
    tr.train()
    return tr


def test_trainer_on_16_bit_noisy_images_without_a_gpu(tmp_path, monkeypatch):
    from PIL import Image
    from ssdn.train import DenoiserTrainer, resume_run
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    f16, f8 = str(tmp_path / "noisy16"), str(tmp_path / "noisy8")
    os.makedirs(f16)
    os.makedirs(f8)
    rs = np.random.RandomState(1)
    arrays = [rs.randint(0, 4096, (h, w)).astype(np.uint16) for h, w in ((40, 48), (33, 70), (20, 36), (64, 32))]
    for k, a in enumerate(arrays):
        Image.fromarray(a).save(os.path.join(f16, "im%d.png" % k))
        Image.fromarray((a >> 4).astype(np.uint8)).save(os.path.join(f8, "im%d.png" % k))
    tr = _train(tmp_path, f16, "runs", white=4095)
    assert isinstance(tr.trainloader, DevicePoolStream) and tr.trainloader.pool.bits == 16 and tr.trainloader.pool.white == 4095
    for idx, inp in tr.denoiser.batches:
        assert inp.shape == (4, 1, 32, 32)
        for b, i in enumerate(idx):                    # every patch is made of its own image's samples at this white level
            assert set(np.unique(inp[b].numpy())) <= set(np.unique(R.sample_in(arrays[i], 4095)))
    last = os.path.join("training", "model_00000008.training")
    sd = torch.load(os.path.join(tr.run_dir_path, last), map_location="cpu", weights_only=False)
    assert sd["noisy"] == {"mode": "style", "augment": False, "pool_bytes": None, "white": 4095}
    # without white -- 16-bit at the default, and an 8-bit run -- the key holds exactly what it held
    for folder, runs in ((f16, "runs_d"), (f8, "runs8")):
        t0 = _train(tmp_path, folder, runs)
        sd0 = torch.load(os.path.join(t0.run_dir_path, last), map_location="cpu", weights_only=False)
        assert sd0["noisy"] == {"mode": "style", "augment": False, "pool_bytes": None} and set(sd0) == set(sd)
    r = resume_run(tr.run_dir_path, 4)
    assert r.noisy == "style" and r.white == 4095
    assert resume_run(t0.run_dir_path).white is None
    # what only the built pool can refuse
    for folder, noisy, white, text in ((f8, "style", 255, "white is the white level of a 16-bit pool"),
                                       (f16, "auto", None, "--noisy auto with 16-bit training images")):
        bad = DenoiserTrainer(_cfg(), runs_dir=str(tmp_path / "runs_bad"))
        bad.noisy, bad.white = noisy, white
        bad.set_train_data(folder)
        with pytest.raises(ValueError, match=text):
            bad.train_data()
