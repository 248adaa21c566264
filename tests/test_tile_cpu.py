"""No GPU: the tiling of SSDN_OP_TILE_IN / SSDN_OP_TILE_OUT as tests/tile_ref.py models it -- the grid's properties, the tiles against
np.pad, the identity that tiles cut from one picture blend back to that picture, the blend weights --, the C ABI of the two ops and their
host-side refusals, and the `tile` / `overlap` options of `ssdn denoise` and `Denoiser.denoise` that are refused before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import tile_ref as TR
from ssdn.hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the grid ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,O", TR.GRIDS)
def test_grid_properties(T, O):
    S = T - O
    for n in range(1, 3 * T + 6):
        K, org = TR.count(n, T, O), TR.origins(n, T, O)
        assert K == len(org) == L.tile_count(n, T, O)
        assert all(o % 32 == 0 for o in org)
        assert (K == 1) == (n <= T)
        assert org[-1] + T >= n                                             # the last tile ends at or beyond n
        assert K == 1 or org[-1] < n                                        # ... and no tile starts beyond the axis
        cov = np.zeros(n, dtype=np.int64)
        for o in org:
            cov[o:min(o + T, n)] += 1
        assert cov.min() >= 1 and cov.max() <= 2                            # one or two tiles, never three
        for a, b in zip(org, org[1:]):
            assert a + T - b == O                                           # neighbours overlap by exactly O
        # the arithmetic cover names exactly the tiles that hold a position -- except in the last tile's surplus overlap, where the
        # definition takes the last tile alone
        two, ka, la, kb, lb, t = TR.cover(n, T, O)
        p = np.arange(n)
        assert ((0 <= la) & (la < T) & (0 <= lb) & (lb < T)).all()
        assert (ka * S + la == p).all() and (kb * S + lb == p).all()
        assert (ka == np.where(two, kb - 1, kb)).all() and (two == (t > 0)).all()
        assert ((cov == 2) >= two).all()


# ---- 2. tile_in against np.pad ------------------------------------------------------------------------------------------------------------------
def _tiles_by_pad(img, T, O):
    h, w, Cn = img.shape
    S = T - O
    Kx, Ky = TR.count(w, T, O), TR.count(h, T, O)
    full_w, full_h = (Kx - 1) * S + T, (Ky - 1) * S + T
    p = np.pad(img, ((0, full_h - h), (0, full_w - w), (0, 0)), mode="reflect")
    x = p.astype(np.float32) / np.float32(255.0)
    return np.stack([x[ky * S:ky * S + T, kx * S:kx * S + T].transpose(2, 1, 0) for ky in range(Ky) for kx in range(Kx)])


@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("T,O", TR.GRIDS)
@pytest.mark.parametrize("h,w", TR.SIZES + [(1, 1), (2, 37), (3, 2), (37, 3), (1, 150)])
def test_tile_in_of_the_model_is_pad_and_slice(h, w, T, O, Cn):
    """includes pads longer than the axis: n in {1, 2, 3, 37} with T = 64"""
    img = TR.make_image(h, w, Cn, seed=h * 7 + w)
    got, want = TR.tile_in_ref(img, T, O), _tiles_by_pad(img, T, O)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # a range of tiles is that range of all tiles
    n = got.shape[0]
    if n > 1:
        assert np.array_equal(TR.tile_in_ref(img, T, O, k0=1, B=n - 1), got[1:])


@pytest.mark.parametrize("n", [1, 2, 3, 37])
def test_reflect_longer_than_the_axis(n):
    a = np.arange(n)
    assert np.array_equal(TR.reflect(np.arange(64), n), np.pad(a, (0, 64 - n), mode="reflect"))


# ---- 3. the identity ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("T,O", TR.GRIDS)
@pytest.mark.parametrize("h,w", TR.SIZES)
def test_tiles_of_one_picture_blend_back_to_it(h, w, T, O, Cn):
    img = TR.make_image(h, w, Cn, seed=h + w + T)
    store = TR.tile_in_ref(img, T, O)
    assert np.array_equal(TR.tile_out_ref(store, w, h, T, O, 0), img)
    exact = (img.astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1)
    got = TR.tile_out_ref(store, w, h, T, O, 1)
    assert got.shape == (Cn, h, w) and np.array_equal(got.view(np.uint32), exact.view(np.uint32))


def test_single_tiles_pass_untouched_and_nan_propagates():
    """a position under one tile is that tile's bits -- inf, NaN and -0.0 included, which a lerp(a, a, t) would not return"""
    T, O, w, h = 64, 32, 100, 70
    store = TR.make_store(TR.count(w, T, O) * TR.count(h, T, O), 1, T, seed=2)
    store[0, 0, 3, 5], store[0, 0, 4, 5], store[0, 0, 5, 5] = np.inf, np.nan, -0.0
    v = TR.blend_ref(store, w, h, T, O)
    assert np.array_equal(v[0, :32, :32].view(np.uint32), store[0, 0, :32, :32].T.view(np.uint32))
    # blended: NaN in either tile gives NaN, and q(NaN) = 0
    store[:] = 0.5
    store[1, 0, 2, 7] = np.nan                       # tile kx = 1 at local x = 2: image x = 34, blended with tile 0
    v = TR.blend_ref(store, w, h, T, O)
    assert np.isnan(v[0, 7, 34]) and np.isnan(v).sum() == 1
    assert TR.tile_out_ref(store, w, h, T, O, 0)[7, 34, 0] == 0


# ---- 4. the weights -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("O", [32, 64, 96, 128])
def test_weights(O):
    d = np.arange(O)
    t = TR.weight(d, O)
    assert t.dtype == np.float32 and (t > 0).all() and (t < 1).all() and (np.diff(t) > 0).all()
    # symmetric to rounding: t(d) + t(O - 1 - d) = 1 within an ulp of 1
    assert np.abs((t + t[::-1]).astype(np.float64) - 1).max() <= 2.0 ** -23
    assert np.array_equal(t, ((2 * d + 1) / (2 * O)).astype(np.float32))            # (the exact quotient, rounded once)
    # two tiles holding the constants 0 and 1 blend to t itself
    T = 2 * O
    w, h = T + 5, 8
    store = np.zeros((2, 1, T, T), dtype=np.float32)
    store[1] = 1
    v = TR.blend_ref(store, w, h, T, O)
    assert np.array_equal(v[0, 0, O:2 * O], t) and (v[0, :, :O] == 0).all() and (v[0, :, 2 * O:] == 1).all()


# ---- 5. the C ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_struct_size():
    hdr = open(os.path.join(ROOT, "include", "ssdn_hip.h")).read()
    assert re.search(r"SSDN_OP_TILE_IN\s*=\s*32\b", hdr) and re.search(r"SSDN_OP_TILE_OUT\s*=\s*33\b", hdr)
    assert "} ssdn_tile_in_args;" in hdr and "} ssdn_tile_out_args;" in hdr
    assert re.search(r"#define SSDN_ABI_VERSION 19\b", hdr) and L.ABI_VERSION == 19
    assert L.OP["tile_in"] == 32 and L.OP["tile_out"] == 33
    assert L.ARG_TYPES["tile_in"] is L.TileInArgs and L.ARG_TYPES["tile_out"] is L.TileOutArgs
    assert [n for n, _ in L.TileInArgs._fields_] == ["src", "src_bytes", "w", "h", "C", "T", "O", "Kx", "Ky", "k0", "B", "dst"]
    assert [n for n, _ in L.TileOutArgs._fields_] == ["store", "w", "h", "C", "T", "O", "Kx", "Ky", "mode", "dst", "dst_bytes"]
    lib = L.load()
    assert lib.ssdn_struct_size(32) == C.sizeof(L.TileInArgs) == 64
    assert lib.ssdn_struct_size(33) == C.sizeof(L.TileOutArgs) == 56


def test_planned_lists_know_nothing_of_the_ops():
    for f in (("selfsupervised-denoising_amd", "ssdn", "hip", "graph.py"), ("oracle", "interp.py")):
        assert "tile_in" not in open(os.path.join(ROOT, *f)).read().lower()


def _refused(op, **kw):
    """run one op with dummy (never dereferenced) pointers -> the library's error text; a well-formed 100 x 70 image at (64, 32) otherwise"""
    if op == "tile_in":
        f = dict(src=0x1000, src_bytes=100 * 70 * 3, w=100, h=70, C=3, T=64, O=32, Kx=3, Ky=2, k0=0, B=2, dst=0x1000)
    else:
        f = dict(store=0x1000, w=100, h=70, C=3, T=64, O=32, Kx=3, Ky=2, mode=0, dst=0x1000, dst_bytes=100 * 70 * 3)
    f.update(kw)
    a = L.ARG_TYPES[op](**f)
    rec = (L.OpRec * 1)()
    rec[0].type, rec[0].lane, rec[0].args = L.OP[op], 0, C.cast(C.pointer(a), C.c_void_p)
    lib = L.load()
    assert lib.ssdn_run_ops(rec, 1, None) != 0
    return lib.ssdn_last_error().decode()


_WIDE = 32 * 65535 + 1          # an axis of 65536 tiles of 32, and of 65536 patches of 32
_COMMON = [(dict(dst=None), "must be given"),
           (dict(C=2), "C must be 1 or 3"), (dict(C=0), "C must be 1 or 3"), (dict(C=4), "C must be 1 or 3"),
           (dict(w=0), "w and h must be at least 1"), (dict(h=-1), "w and h must be at least 1"),
           (dict(T=0), "T must be a positive multiple of 32"), (dict(T=48), "T must be a positive multiple of 32"),
           (dict(T=-64), "T must be a positive multiple of 32"),
           (dict(O=-32), "O must be a multiple of 32"), (dict(O=16), "O must be a multiple of 32"), (dict(O=64), "0 <= 2 O <= T"),
           (dict(Kx=2), "the grid must be Kx = 3, Ky = 2"), (dict(Ky=3), "the grid must be Kx = 3, Ky = 2"),
           (dict(Kx=1, Ky=1, T=32, O=0), "the grid must be Kx = 4, Ky = 3"),
           (dict(w=1 << 16, h=1 << 15, C=1, T=1 << 16, O=0, Kx=1, Ky=1), "w h C must be below 2\\^31")]


@pytest.mark.parametrize("kw,msg", _COMMON + [
    (dict(src=None), "must be given"), (dict(B=0), "inside the grid"), (dict(k0=-1), "inside the grid"), (dict(k0=5, B=2), "inside the grid"),
    (dict(k0=6, B=1), "inside the grid"), (dict(src_bytes=100 * 70 * 3 - 1), "src_bytes is below"),
    (dict(w=_WIDE, h=1, C=1, T=32, O=0, Kx=65536, Ky=1, B=65536, src_bytes=_WIDE), "at most 65535")])
def test_tile_in_refuses_bad_arguments_without_a_gpu(kw, msg):
    err = _refused("tile_in", **kw)
    assert re.search(r"^op 0 \(type 32\): tile_in: .*" + msg, err), err


@pytest.mark.parametrize("kw,msg", _COMMON + [
    (dict(store=None), "must be given"), (dict(mode=2), "mode must be 0"), (dict(mode=-1), "mode must be 0"),
    (dict(dst_bytes=100 * 70 * 3 - 1), "dst_bytes is below"), (dict(mode=1), "dst_bytes is below"),
    (dict(w=_WIDE, h=1, C=1, T=32, O=0, Kx=65536, Ky=1, dst_bytes=_WIDE), "at most 65535")])
def test_tile_out_refuses_bad_arguments_without_a_gpu(kw, msg):
    err = _refused("tile_out", **kw)
    assert re.search(r"^op 0 \(type 33\): tile_out: .*" + msg, err), err


# ---- 6. the command and the method's refusals -----------------------------------------------------------------------------------------------------
def test_cli_denoise_tile_flags():
    from ssdn.cli.cli import build_parser
    parser, _ = build_parser()
    a = vars(parser.parse_args(["denoise", "-m", "x.wt", "-i", "imgs", "-o", "out"]))
    assert a["tile"] is None and a["overlap"] is None
    b = vars(parser.parse_args(["denoise", "-m", "x.wt", "-i", "imgs", "-o", "out", "--tile", "512", "--overlap", "64"]))
    assert (b["tile"], b["overlap"]) == (512, 64)


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


_BAD = [(dict(overlap=32), "overlap needs tile"), (dict(tile=48), "tile must be a positive multiple of 32"),
        (dict(tile=0), "tile must be a positive multiple of 32"), (dict(tile=-64), "tile must be a positive multiple of 32"),
        (dict(tile=64, overlap=48), "overlap must be a multiple of 32"), (dict(tile=64, overlap=-32), "overlap must be a multiple of 32"),
        (dict(tile=64, overlap=64), "2 \\* overlap"), (dict(tile=96, overlap=64), "2 \\* overlap")]


def test_denoise_tile_refusals_need_no_device():
    from ssdn.params import NoiseAlgorithm, NoiseValue
    known = _cpu_denoiser(NoiseAlgorithm.SELFSUPERVISED_DENOISING, "gauss25", NoiseValue.KNOWN)
    n2c = _cpu_denoiser(NoiseAlgorithm.NOISE_TO_CLEAN, "gauss25")
    rgb = np.zeros((80, 90, 3), dtype=np.uint8)
    for kw, msg in _BAD:
        with pytest.raises(ValueError, match=msg):
            known.denoise([rgb], noise_param=25, **kw)
        with pytest.raises(ValueError, match=msg):
            n2c.denoise([rgb], **kw)
    assert known.denoise([], noise_param=25, tile=64) == {"out": [], "noise_std": [], "tiles": []}


def test_default_overlap():
    from ssdn.denoiser import Denoiser
    want = {32: 0, 64: 32, 96: 32, 128: 32, 160: 32, 256: 64, 512: 128, 544: 128, 1024: 256}
    for T, O in want.items():
        assert Denoiser._tile_options(T, None) == (T, O), T
        TR.check(T, O)
    assert Denoiser._tile_options(None, None) == (None, None)
    assert Denoiser._tile_options(128, 0) == (128, 0) and Denoiser._tile_options(128, 64) == (128, 64)


def test_cli_refuses_tile_options_before_a_file_is_opened(tmp_path):
    from ssdn.__main__ import start_cli
    from ssdn.params import NoiseAlgorithm
    d = _cpu_denoiser(NoiseAlgorithm.NOISE_TO_CLEAN, "gauss25")
    torch.save({k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in d.state_dict().items()}, tmp_path / "n2c.wt")
    io = ["-m", str(tmp_path / "n2c.wt"), "-i", str(tmp_path / "none"), "-o", str(tmp_path / "out")]
    for flags, msg in ((["--overlap", "32"], "overlap needs tile"), (["--tile", "48"], "tile must be a positive multiple of 32"),
                       (["--tile", "64", "--overlap", "48"], "overlap must be a multiple of 32"),
                       (["--tile", "64", "--overlap", "64"], "2 \\* overlap")):
        with pytest.raises(ValueError, match=msg):
            start_cli(["denoise"] + io + flags)
    assert not os.path.exists(tmp_path / "out")
