"""No GPU: the numpy model of SSDN_OP_IMAGE_IN / SSDN_OP_IMAGE_OUT (tests/image_io_ref.py) against the package's host route, bit for bit; the
quantiser on its edges; the C ABI of the two ops and their host-side refusals; `ssdn denoise`'s parser and the refusals of
`Denoiser.denoise` that come before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import image_io_ref as IO
from ssdn.hip import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the model against the host route ----------------------------------------------------------------------------------------------------
def _clamped(H, W):
    """EXTENTS inside a padded tensor of H x W: an extent the tensor cannot hold is cut to it (the host route cannot pad by a negative
    amount), so 32 x 96 runs (1,1), (2,2), (5,37), (32,1), (32,64), (32,64)"""
    return [(min(e1, H), min(e2, W)) for e1, e2 in IO.EXTENTS]


@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("H,W", IO.PADDED)
def test_model_is_the_host_route_bit_for_bit(H, W, Cn):
    """in: to_tensor, permute, pad_to_output_size; out: unpad, tensor2image -- of a tensor that is NOT k/255 everywhere, so the
    quantiser's truncation is exercised"""
    ext = _clamped(H, W)
    images = IO.make_images(ext, Cn, seed=H + Cn)
    buf, offs = IO.pack(images)
    got = IO.image_in_ref(buf, buf.size, offs, ext, Cn, H, W)
    want = IO.host_in(images, H, W).numpy()
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape == (len(ext), Cn, H, W)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # out: a denoiser-like tensor -- the padded input plus something smooth, beyond [0, 1] in places
    g = np.random.default_rng(7)
    x = (want * np.float32(1.2) - np.float32(0.1) + g.normal(0, 0.01, want.shape).astype(np.float32)).astype(np.float32)
    dst = np.full(buf.size, IO.GUARD_BYTE, dtype=np.uint8)
    IO.image_out_ref(x, ext, offs, dst, dst.size)
    for b, a in enumerate(IO.host_out(torch.from_numpy(x), images)):
        h, w = images[b].shape[:2]
        assert np.array_equal(dst[offs[b]:offs[b] + h * w * Cn].reshape(h, w, Cn), a), (b, ext[b])
    # nothing outside the images: the guard bytes are what they were
    mask = np.ones(buf.size, dtype=bool)
    for b, im in enumerate(images):
        mask[offs[b]:offs[b] + im.size] = False
    assert mask.sum() == IO.GUARD * (len(images) + 1) and (dst[mask] == IO.GUARD_BYTE).all()


@pytest.mark.parametrize("n", [1, 2, 3, 5, 37, 64])
def test_reflect_is_numpys_for_any_pad_length(n):
    a = np.arange(n)
    for total in (32, 64, 96):
        if total >= n:
            assert np.array_equal(IO.reflect(np.arange(total), n), np.pad(a, (0, total - n), mode="reflect"))


@pytest.mark.parametrize("Cn", [1, 3])
def test_round_trip_of_every_byte(Cn):
    """out(in(u8)) == u8 for all 256 byte values, wherever they lie in an odd-sized image"""
    h, w = 11, 24
    im = (np.arange(h * w * Cn) * 7 % 256).astype(np.uint8).reshape(h, w, Cn)
    assert len(np.unique(im)) == 256
    buf, offs = IO.pack([im])
    x = IO.image_in_ref(buf, buf.size, offs, [(w, h)], Cn, 32, 32)
    dst = np.zeros_like(buf)
    IO.image_out_ref(x, [(w, h)], offs, dst, dst.size)
    assert np.array_equal(dst[offs[0]:offs[0] + im.size].reshape(h, w, Cn), im)
    assert np.array_equal(IO.quantise(np.arange(256, dtype=np.float32) / np.float32(255.0)), np.arange(256, dtype=np.uint8))


def test_quantiser_on_its_edges():
    k = np.arange(256, dtype=np.float32) / np.float32(255.0)
    up, down = np.nextafter(k, np.float32(2)), np.nextafter(k, np.float32(-1))
    for v in (k, up, down):
        want = np.uint8(np.clip(v, 0, 1) * np.float32(255.0))               # tensor2image's expression
        assert np.array_equal(IO.quantise(v), want)
    assert np.array_equal(IO.quantise(k), np.arange(256, dtype=np.uint8))
    assert (IO.quantise(up) >= np.arange(256)).all() and (IO.quantise(down) <= np.arange(256)).all()
    edge = np.array([-0.0, -1e-30, -1.0, -3e38, 1.0, 1.0000001, 2.0, 3e38, np.inf, -np.inf, np.nan, 0.999999, 0.5], dtype=np.float32)
    assert IO.quantise(edge).tolist() == [0, 0, 0, 0, 255, 255, 255, 255, 255, 0, 0, 254, 127]
    g = np.random.default_rng(3)
    v = g.uniform(-0.2, 1.2, 1 << 16).astype(np.float32)
    assert np.array_equal(IO.quantise(v), np.uint8(np.clip(v, 0, 1) * np.float32(255.0)))


def test_inconsistent_tables_in_the_model():
    """an extent beyond the tensor is clamped; an offset past the buffer reads zeros and writes nothing; an empty extent is zeros / nothing"""
    im = IO.make_images([(8, 8)], 3, seed=1)[0]
    buf, offs = IO.pack([im, im, im, im])
    ext = [(8, 8), (999, -4), (8, 8), (8, 8)]
    offs = [offs[0], offs[1], buf.size - 10, -5]
    x = IO.image_in_ref(buf, buf.size, offs, ext, 3, 32, 32)
    assert (x[1] == 0).all() and (x[3] == 0).all()
    assert np.count_nonzero(x[2]) <= 10 * 32 * 32 and (x[2].reshape(3, -1)[:, 32 * 8:] >= 0).all()
    dst = np.full(buf.size, 0xAB, dtype=np.uint8)
    IO.image_out_ref(np.ones((4, 3, 32, 32), dtype=np.float32), ext, offs, dst, dst.size)
    changed = np.flatnonzero(dst != 0xAB)
    assert set(changed) == set(range(offs[0], offs[0] + 192)) | set(range(buf.size - 10, buf.size))


# ---- 2. the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_struct_size():
    hdr = open(os.path.join(ROOT, "include", "ssdn_hip.h")).read()
    assert re.search(r"SSDN_OP_IMAGE_IN\s*=\s*29\b", hdr) and re.search(r"SSDN_OP_IMAGE_OUT\s*=\s*30\b", hdr)
    assert "} ssdn_image_in_args;" in hdr and "} ssdn_image_out_args;" in hdr
    assert re.search(r"#define SSDN_ABI_VERSION 19\b", hdr) and L.ABI_VERSION == 19
    assert L.OP["image_in"] == 29 and L.OP["image_out"] == 30
    assert L.ARG_TYPES["image_in"] is L.ImageInArgs and L.ARG_TYPES["image_out"] is L.ImageOutArgs
    assert [n for n, _ in L.ImageInArgs._fields_] == ["src", "src_bytes", "offs", "ext", "B", "C", "H", "W", "dst"]
    assert [n for n, _ in L.ImageOutArgs._fields_] == ["x", "ext", "offs", "dst", "dst_bytes", "B", "C", "H", "W"]
    lib = L.load()
    assert lib.ssdn_struct_size(29) == C.sizeof(L.ImageInArgs) == 56
    assert lib.ssdn_struct_size(30) == C.sizeof(L.ImageOutArgs) == 56
    # every op name of the enum stays letters and underscores (tests/test_abi.py reads it that way)
    assert {"IMAGE_IN", "IMAGE_OUT"} <= set(re.findall(r"SSDN_OP_([A-Z_]+)\s*=", hdr))


def _refused(op, **kw):
    """run one op with dummy (never dereferenced) pointers -> the library's error text"""
    if op == "image_in":
        f = dict(src=0x1000, src_bytes=64, offs=0x1000, ext=0x1000, B=1, C=3, H=32, W=32, dst=0x1000)
    else:
        f = dict(x=0x1000, ext=0x1000, offs=0x1000, dst=0x1000, dst_bytes=64, B=1, C=3, H=32, W=32)
    f.update(kw)
    a = L.ARG_TYPES[op](**f)
    rec = (L.OpRec * 1)()
    rec[0].type, rec[0].lane, rec[0].args = L.OP[op], 0, C.cast(C.pointer(a), C.c_void_p)
    lib = L.load()
    assert lib.ssdn_run_ops(rec, 1, None) != 0
    return lib.ssdn_last_error().decode()


_COMMON = [(dict(offs=None), "must be given"), (dict(ext=None), "must be given"), (dict(dst=None), "must be given"),
           (dict(C=2), "C must be 1 or 3"), (dict(C=0), "C must be 1 or 3"), (dict(C=4), "C must be 1 or 3"),
           (dict(B=0), "B, H and W must be at least 1"), (dict(H=0), "B, H and W must be at least 1"),
           (dict(W=-1), "B, H and W must be at least 1"), (dict(B=65536), "at most 65535"), (dict(H=32 * 65535 + 1), "at most 65535")]


@pytest.mark.parametrize("kw,msg", _COMMON + [(dict(src=None), "must be given"), (dict(src_bytes=-1), "byte count must not be negative")])
def test_image_in_refuses_bad_arguments_without_a_gpu(kw, msg):
    err = _refused("image_in", **kw)
    assert re.search(r"^op 0 \(type 29\): image_in: .*" + msg, err), err


@pytest.mark.parametrize("kw,msg", _COMMON + [(dict(x=None), "must be given"), (dict(dst_bytes=-1), "byte count must not be negative")])
def test_image_out_refuses_bad_arguments_without_a_gpu(kw, msg):
    err = _refused("image_out", **kw)
    assert re.search(r"^op 0 \(type 30\): image_out: .*" + msg, err), err


def test_planned_lists_know_nothing_of_the_ops():
    for f in (("selfsupervised-denoising_amd", "ssdn", "hip", "graph.py"), ("oracle", "interp.py")):
        assert "image_in" not in open(os.path.join(ROOT, *f)).read().lower()


# ---- 3. the command and the method's refusals -------------------------------------------------------------------------------------------------
def test_cli_denoise_flags():
    from ssdn.cli.cli import build_parser
    parser, cmds = build_parser()
    assert set(cmds) == {"train", "eval", "denoise"}
    a = vars(parser.parse_args(["denoise", "-m", "x.wt", "-i", "imgs", "-o", "out"]))
    assert (a["model"], a["input"], a["output"]) == ("x.wt", "imgs", "out")
    assert a["noise_param"] is None and a["batch_size"] == 1 and a["bucket"] is None
    assert a["uniform"] is False and a["std"] is False and a["recursive"] is False
    b = vars(parser.parse_args(["denoise", "--model", "x.wt", "--input", "imgs", "--output", "out", "--noise_param", "25", "--batch_size", "4",
                                "--bucket", "64", "--uniform", "--std", "--recursive"]))
    assert (b["noise_param"], b["batch_size"], b["bucket"], b["uniform"], b["std"], b["recursive"]) == ("25", 4, 64, True, True, True)


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


def test_cli_refuses_the_noise_parameter_mismatch_before_any_device_call(tmp_path):
    """a known-sigma model without --noise_param, a const model with one: ValueError before a file is read or a directory made"""
    from ssdn.__main__ import start_cli
    from ssdn.params import NoiseAlgorithm, NoiseValue
    _save(_cpu_denoiser(NoiseAlgorithm.SELFSUPERVISED_DENOISING, "gauss25", NoiseValue.KNOWN), tmp_path / "known.wt")
    _save(_cpu_denoiser(NoiseAlgorithm.SELFSUPERVISED_DENOISING, "gauss25", NoiseValue.UNKNOWN_CONSTANT), tmp_path / "const.wt")
    io = ["-i", str(tmp_path / "none"), "-o", str(tmp_path / "out")]
    with pytest.raises(ValueError, match="noise_param is required"):
        start_cli(["denoise", "-m", str(tmp_path / "known.wt")] + io)
    with pytest.raises(ValueError, match="this model takes none"):
        start_cli(["denoise", "-m", str(tmp_path / "const.wt"), "--noise_param", "25"] + io)
    assert not os.path.exists(tmp_path / "out")


def test_denoise_refusals_need_no_device():
    from ssdn.params import NoiseAlgorithm, NoiseValue
    known = _cpu_denoiser(NoiseAlgorithm.SELFSUPERVISED_DENOISING, "gauss25", NoiseValue.KNOWN)
    rgb, gray = np.zeros((8, 9, 3), dtype=np.uint8), np.zeros((8, 9), dtype=np.uint8)
    with pytest.raises(ValueError, match="has 1 channel"):
        known.denoise([rgb, gray], noise_param=25)
    with pytest.raises(ValueError, match="has 3 channel"):
        _cpu_denoiser(NoiseAlgorithm.NOISE_TO_CLEAN, "gauss25", channels=1).denoise([rgb])
    for bad in (48, 0, -32, 33):
        with pytest.raises(ValueError, match="bucket must be a positive multiple of 32"):
            known.denoise([rgb], noise_param=25, bucket=bad)
    with pytest.raises(ValueError, match="noise_param is required"):
        known.denoise([rgb])
    with pytest.raises(ValueError, match="not one number"):
        known.denoise([rgb], noise_param="5_50")
    with pytest.raises(ValueError, match="uint8"):
        known.denoise([rgb.astype(np.float32)], noise_param=25)
    n2c = _cpu_denoiser(NoiseAlgorithm.NOISE_TO_CLEAN, "gauss25")
    with pytest.raises(ValueError, match="this model takes none"):
        n2c.denoise([rgb], noise_param=25)
    with pytest.raises(ValueError, match="std=True"):
        n2c.denoise([rgb], std=True)
    assert known.denoise([], noise_param=25) == {"out": [], "noise_std": []} and n2c.denoise([]) == {"out": []}


def test_noise_param_grammar():
    from ssdn.params import NoiseAlgorithm, NoiseValue
    A, K = NoiseAlgorithm.SELFSUPERVISED_DENOISING, NoiseValue.KNOWN
    g = _cpu_denoiser(A, "gauss25", K)
    assert g._noise_param_value(25) == g._noise_param_value("25") == 25 / 255 and g._noise_param_value(0.1) == g._noise_param_value("0.1") == 0.1
    assert _cpu_denoiser(A, "poisson30", K)._noise_param_value(30) == 30.0
    i = _cpu_denoiser(A, "impulse50", K)
    assert i._noise_param_value(50) == 0.5 and i._noise_param_value("0.25") == 0.25
