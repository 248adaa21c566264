"""CPU: SSIM (ssdn.utils.calculate_ssim, SSDN_OP_SSIM, `ssdn eval --ssim`): the float64 specification against an independent scipy
implementation and against closed forms, the C ABI of the op and its argument rules (raised before any device call, so they show without
a GPU), and the opt-in switches of the trainer and the command line."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from ssdn.hip import lib as L
from ssdn.utils import calculate_ssim
from ssim_ref import make_pair, ssim_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the specification -------------------------------------------------------------------------------------------------------------------
def test_specification_against_scipy():
    x, ref = make_pair(2, 3, 37, 45)
    val, smap = calculate_ssim(x, ref, full=True)
    rv, rmap = ssim_ref(x, ref)
    assert val.dtype == torch.float32 and smap.dtype == torch.float64 and tuple(smap.shape) == (2, 3, 27, 35)
    err = float((smap - torch.from_numpy(rmap)).abs().max())
    print("map error against scipy: %.3e" % err)
    assert err <= 1e-10
    assert float((val.double() - torch.from_numpy(rv)).abs().max()) <= 6e-8          # (the float32 rounding of the value)
    assert float(smap.min()) < 0 < float(smap.max()) <= 1 + 1e-12                      # the x = 1 - ref region is there


@pytest.mark.parametrize("a,b", [(0.5, 0.6), (0.0, 1.0), (0.25, 0.25)])
def test_two_constant_images_have_a_closed_form(a, b):
    x, y = torch.full((1, 3, 16, 19), a), torch.full((1, 3, 16, 19), b)
    fa, fb = float(x[0, 0, 0, 0]), float(y[0, 0, 0, 0])
    want = (2 * fa * fb + 1e-4) / (fa * fa + fb * fb + 1e-4)
    val, smap = calculate_ssim(x, y, full=True)
    assert float((smap - want).abs().max()) <= 1e-12 and abs(float(val[0]) - want) <= 6e-8
    if (a, b) == (0.5, 0.6):
        assert "%.6f" % float(val[0]) == "0.983609"


def test_identity_symmetry_and_layouts():
    x, ref = make_pair(2, 3, 23, 31, seed=1)
    assert torch.equal(calculate_ssim(x, x), torch.ones(2))
    v, m = calculate_ssim(x, ref, full=True)
    v2, m2 = calculate_ssim(ref, x, full=True)
    assert torch.equal(v, v2) and float((m - m2).abs().max()) <= 1e-13
    for b in range(2):                                                             # CHW: a scalar, the BCHW value of that sample
        s, sm = calculate_ssim(x[b], ref[b], full=True)
        assert s.dim() == 0 and torch.equal(s, v[b]) and torch.equal(sm, m[b])


@pytest.mark.parametrize("h,w", [(10, 40), (40, 10), (3, 3)])
def test_below_the_window_is_nan(h, w):
    x, ref = torch.rand(2, 3, h, w), torch.rand(2, 3, h, w)
    v, m = calculate_ssim(x, ref, full=True)
    assert v.shape == (2,) and torch.isnan(v).all() and m.numel() == 0
    assert math.isnan(float(calculate_ssim(x[0], ref[0])))


# ---- 2. the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_struct_size():
    hdr = open(os.path.join(ROOT, "include", "ssdn_hip.h")).read()
    assert re.search(r"SSDN_OP_SSIM\s*=\s*27\b", hdr) and "} ssdn_ssim_args;" in hdr
    assert re.search(r"#define SSDN_ABI_VERSION 19\b", hdr) and L.ABI_VERSION == 19
    assert L.OP["ssim"] == 27 and L.ARG_TYPES["ssim"] is L.SsimArgs
    assert [n for n, _ in L.SsimArgs._fields_] == ["x", "ref", "ext", "B", "C", "H", "W", "ssim", "map", "scratch", "scratch_bytes"]
    assert L.load().ssdn_struct_size(27) == C.sizeof(L.SsimArgs)
    # the scratch rule of the header and the binding's copy of it
    th, tw = (int(re.search(r"#define SSDN_SSIM_TILE_%s (\d+)" % a, hdr).group(1)) for a in "HW")
    assert (th, tw) == (L.SSIM_TILE_H, L.SSIM_TILE_W)
    assert L.ssim_scratch_bytes(2, 3, 11, 11) == 8 * 6 and L.ssim_scratch_bytes(3, 3, 50, 77) == 8 * 9 * -(-40 // th) * -(-67 // tw)


def _refused(**kw):
    """run one op with dummy (never dereferenced) pointers -> the library's error text"""
    f = dict(x=0x1000, ref=0x1000, ext=None, B=1, C=3, H=16, W=16, ssim=0x1000, map=None, scratch=0x1000, scratch_bytes=1 << 20)
    f.update(kw)
    a = L.SsimArgs(**f)
    rec = (L.OpRec * 1)()
    rec[0].type, rec[0].lane, rec[0].args = L.OP["ssim"], 0, C.cast(C.pointer(a), C.c_void_p)
    lib = L.load()
    assert lib.ssdn_run_ops(rec, 1, None) != 0
    return lib.ssdn_last_error().decode()


@pytest.mark.parametrize("kw,msg", [
    (dict(x=None), "x and ref must be given"),
    (dict(ref=None), "x and ref must be given"),
    (dict(ssim=None), "the output ssim must be given"),
    (dict(scratch=None), "scratch must be given"),
    (dict(B=0), "B and C must be at least 1"),
    (dict(C=0), "B and C must be at least 1"),
    (dict(H=10), "H and W must be at least 11"),
    (dict(W=10), "H and W must be at least 11"),
    (dict(scratch_bytes=8 * 3 - 1), "scratch_bytes is below"),
])
def test_run_ops_refuses_bad_arguments_without_a_gpu(kw, msg):
    err = _refused(**kw)
    assert re.search(r"ssim: " + msg, err), err


# ---- 3. the switches ------------------------------------------------------------------------------------------------------------------------
def test_cli_eval_ssim_flag():
    from ssdn.cli.cli import build_parser
    parser, _ = build_parser()
    assert vars(parser.parse_args(["eval", "-m", "x.wt", "-d", "imgs", "--ssim"]))["ssim"] is True
    assert vars(parser.parse_args(["eval", "-m", "x.wt", "-d", "imgs"]))["ssim"] is False


def test_trainer_switch_is_off_by_default_and_no_config_value():
    from ssdn.params import ConfigValue
    from ssdn.train import DenoiserTrainer
    assert DenoiserTrainer({}).ssim is False
    assert not any("ssim" in v.name.lower() for v in ConfigValue)


def test_planned_lists_know_nothing_of_the_op():
    for f in (("selfsupervised-denoising_amd", "ssdn", "hip", "graph.py"), ("oracle", "interp.py")):
        assert "ssim" not in open(os.path.join(ROOT, *f)).read().lower()


def test_trainer_cpu_path_is_the_specification_on_the_unpadded_pairs():
    """DenoiserTrainer.calculate_ssim without a GPU: calculate_ssim on each un-padded pair"""
    import ssdn
    from ssdn.datasets import NoisyDataset
    from ssdn.params import ConfigValue, NoiseAlgorithm, PipelineOutput
    from ssdn.train import DenoiserTrainer
    MD = NoisyDataset.Metadata
    cfg = ssdn.cfg.base()
    cfg[ConfigValue.ALGORITHM] = NoiseAlgorithm.NOISE_TO_CLEAN
    cfg[ConfigValue.NOISE_STYLE] = "gauss25"
    tr = DenoiserTrainer(cfg)
    x, ref = make_pair(2, 3, 32, 32, seed=2)
    out = (x + ref) / 2
    meta = {MD.CLEAN: ref, MD.IMAGE_SHAPE: torch.tensor([[3, 32, 32], [3, 20, 13]])}
    got = tr.calculate_ssim([x, ref, meta], {PipelineOutput.IMG_DENOISED: out})
    assert set(got) == {"ssim_nsy", "ssim_out"}
    for name, img in (("ssim_nsy", x), ("ssim_out", out)):
        want = torch.stack([calculate_ssim(img[0], ref[0]), calculate_ssim(img[1, :, :20, :13], ref[1, :, :20, :13])])
        assert torch.equal(got[name], want) and got[name].dtype == torch.float32
