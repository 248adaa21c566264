"""GPU: SSDN_OP_SSIM (csrc/ssim.hip) against the float64 specification ssdn.utils.calculate_ssim, its map and NaN contracts, the bits it
promises, Denoiser.ssim and `ssdn eval --ssim`.

The bound of every comparison with the specification is atol 1.2e-7, rtol 0: SSIM lies in [-1, 1], the kernel's value is the float64 value
(its own error ~1e-12) rounded once to fp32, at most 6e-8 off; the bound is one fp32 ulp at 1.0."""
import csv
import math
import os

import numpy as np
import pytest
import torch

import restate as R
from head_ops import DEV, P, _nan, run_one
from ssim_ref import make_pair
from ssdn.utils import calculate_ssim

pytestmark = pytest.mark.gpu
ATOL = 1.2e-7

# (B, C, H, W, ext): one position; a few; two or more tiles in both axes with uneven remainders (tiles are 16 x 32 positions) and a padded
# batch whose samples have 40 x 67, 1 x 1 and 13 x 27 positions
SHAPES = [(2, 3, 11, 11, None), (2, 1, 13, 17, None), (3, 3, 50, 77, [(50, 77), (11, 11), (23, 37)])]


def ssim_op(x, ref, ext=None, want_map=True, map_init=None):
    """one SSDN_OP_SSIM launch on device copies -> (ssim [B], map [B,C,H,W] or None), device tensors.  The value buffer and (unless
    map_init is given) the map are NaN before the launch; the scratch holds garbage of its own"""
    from ssdn.hip import lib as L
    B, C, H, W = x.shape
    xd, rd = x.to(DEV, torch.float32).contiguous(), ref.to(DEV, torch.float32).contiguous()
    ed = torch.tensor(ext, dtype=torch.int32, device=DEV).contiguous() if ext is not None else None
    val = _nan(B)
    smap = (_nan(B, C, H, W) if map_init is None else map_init.to(DEV).clone()) if want_map else None
    nbytes = L.ssim_scratch_bytes(B, C, H, W)
    scratch = torch.full((nbytes // 8,), 1e300, dtype=torch.float64, device=DEV)
    run_one("ssim", L.SsimArgs(P(xd), P(rd), P(ed), B, C, H, W, P(val), P(smap), P(scratch), nbytes))
    return val, smap


_CASES = {}


def case(i):
    """inputs, one launch with a map and the specification of shape i: computed once, shared, never modified"""
    if i not in _CASES:
        B, C, H, W, ext = SHAPES[i]
        x, ref = make_pair(B, C, H, W, seed=i)
        val, smap = ssim_op(x, ref, ext)
        exts = ext if ext is not None else [(H, W)] * B
        spec = [calculate_ssim(x[b:b + 1, :, :e1, :e2], ref[b:b + 1, :, :e1, :e2], full=True) for b, (e1, e2) in enumerate(exts)]
        _CASES[i] = dict(x=x, ref=ref, ext=ext, exts=exts, val=val.cpu(), map=smap.cpu(), spec=spec)
    return _CASES[i]


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_op_against_the_float64_specification(i):
    c = case(i)
    for b, (e1, e2) in enumerate(c["exts"]):
        sval, smap = c["spec"][b]
        got = c["map"][b, :, 5:e1 - 5, 5:e2 - 5].double()
        err_m = float((got - smap[0]).abs().max())
        err_v = abs(float(c["val"][b].double()) - float(smap.mean()))
        print("shape %s sample %d: map error %.3e, value error %.3e, ssim %.6f, map min %.3f" % (SHAPES[i][:4], b, err_m, err_v, float(sval[0]), float(smap.min())))
        assert err_m <= ATOL and err_v <= ATOL
        assert abs(float(c["val"][b]) - float(sval[0])) <= ATOL            # ... and the specification's own fp32 value


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_map_writes_exactly_the_window_centres(i):
    c = case(i)
    for b, (e1, e2) in enumerate(c["exts"]):
        want = torch.zeros(c["map"].shape[1:], dtype=torch.bool)
        want[:, 5:e1 - 5, 5:e2 - 5] = True
        assert torch.equal(torch.isfinite(c["map"][b]), want), b


def test_a_sample_without_a_position_is_nan_and_leaves_the_others_alone():
    c = case(2)
    ext = [c["exts"][0], (10, 40), c["exts"][2]]
    val, smap = ssim_op(c["x"], c["ref"], ext)
    val, smap = val.cpu(), smap.cpu()
    assert math.isnan(float(val[1])) and torch.isnan(smap[1]).all()
    for b in (0, 2):
        assert torch.equal(val[b], c["val"][b]) and torch.equal(smap[b].nan_to_num(nan=7.0), c["map"][b].nan_to_num(nan=7.0))
    # extents outside the tensor are clamped to it by the kernel (ext is device memory)
    val2, _ = ssim_op(c["x"], c["ref"], [(1000, 1000), (-3, 40), c["exts"][2]], want_map=False)
    full, _ = ssim_op(c["x"], c["ref"], None, want_map=False)
    assert torch.equal(val2[0], full[0]) and math.isnan(float(val2[1])) and torch.equal(val2[2].cpu(), c["val"][2])


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_bits_repeat_with_and_without_the_map_and_whatever_the_padding(i):
    c = case(i)
    again, amap = ssim_op(c["x"], c["ref"], c["ext"])
    assert torch.equal(again.cpu(), c["val"]) and torch.equal(amap.cpu().nan_to_num(nan=7.0), c["map"].nan_to_num(nan=7.0))
    bare, _ = ssim_op(c["x"], c["ref"], c["ext"], want_map=False)
    assert torch.equal(bare.cpu(), c["val"])
    # a map that held numbers keeps them outside the centres
    init = torch.full(c["map"].shape, 3.0)
    _, kept = ssim_op(c["x"], c["ref"], c["ext"], map_init=init)
    assert torch.equal(kept.cpu(), torch.where(torch.isfinite(c["map"]), c["map"], init))
    for b, (e1, e2) in enumerate(c["exts"]):                                 # sample b alone, un-padded and contiguous
        alone, _ = ssim_op(c["x"][b:b + 1, :, :e1, :e2], c["ref"][b:b + 1, :, :e1, :e2], None, want_map=False)
        assert torch.equal(alone.cpu()[0], c["val"][b]), b


# ---- Denoiser.ssim --------------------------------------------------------------------------------------------------------------------------
SIZES = [(40, 24), (32, 32)]                       # un-padded extents of the two images; the batch is padded to 64 x 64


def _eval_batch(seed=0, S=64):
    """a two-image evaluation batch as the padded test loader hands it out: images stored top-left, IMAGE_SHAPE metadata"""
    from ssdn.datasets import NoisyDataset
    MD = NoisyDataset.Metadata
    clean = R.hash_tensor((2, 3, S, S), 161 + seed, 0, 1)
    noisy = clean + R.hash_tensor((2, 3, S, S), 162 + seed, -1, 1) * 0.17
    meta = {MD.CLEAN: clean, MD.INPUT_NOISE_VALUES: torch.full((2, 1, 1, 1), 25 / 255.0),
            MD.IMAGE_SHAPE: torch.tensor([[3, h, w] for h, w in SIZES]), MD.INDEXES: torch.tensor([0, 1])}
    return [noisy.to(DEV), clean.to(DEV), meta]


def test_denoiser_ssim_is_the_specification_on_the_engines_outputs():
    from ssdn.datasets import NoisyDataset
    from ssdn.params import PipelineOutput as PO
    from test_hip_posterior import _denoiser
    d = _denoiser("gauss25", "known", 3)
    with pytest.raises(RuntimeError, match="preceding run_pipeline"):
        d.ssim(_eval_batch())
    data = _eval_batch()
    d.eval()
    with torch.no_grad():
        out = d.run_pipeline(data)
    res = d.ssim(data, maps=True)
    assert set(res) == {"ssim_nsy", "ssim_out", "ssim_mu_out", "map_nsy", "map_out", "map_mu_out"}
    MD = NoisyDataset.Metadata
    clean = data[2][MD.CLEAN]
    for name, img in (("nsy", data[0]), ("out", out[PO.IMG_DENOISED]), ("mu_out", out[PO.IMG_MU])):
        val, smap = res["ssim_" + name], res["map_" + name]
        assert val.dtype == torch.float32 and val.device.type == "cpu" and val.shape == (2,) and smap.shape == (2, 3, 64, 64)
        for b, (h, w) in enumerate(SIZES):
            sv, sm = calculate_ssim(img[b, :, :h, :w].cpu(), clean[b, :, :h, :w], full=True)
            err = abs(float(val[b].double()) - float(sm.mean()))
            merr = float((smap[b, :, 5:h - 5, 5:w - 5].double() - sm).abs().max())
            print("%s sample %d: ssim %.6f, value error %.3e, map error %.3e" % (name, b, float(val[b]), err, merr))
            assert err <= ATOL and merr <= ATOL and abs(float(val[b]) - float(sv)) <= ATOL
            outside = smap[b].clone()
            outside[:, 5:h - 5, 5:w - 5] = 0
            assert not outside.any()
    assert set(d.ssim(data)) == {"ssim_nsy", "ssim_out", "ssim_mu_out"}
    # refusals: no clean image; an extent below the window (decided on the host from the metadata)
    with pytest.raises(ValueError, match="no clean image"):
        d.ssim([data[0], data[1], {k: v for k, v in data[2].items() if k != MD.CLEAN}])
    small = dict(data[2])
    small[MD.IMAGE_SHAPE] = torch.tensor([[3, 40, 24], [3, 10, 32]])
    with pytest.raises(ValueError, match="below the 11 x 11 window"):
        d.ssim([data[0], data[1], small])


def test_denoiser_ssim_changes_nothing_else():
    """outputs, the metric accumulator, the plan blob, a second run_pipeline and three train_steps: bit for bit what they are without the call"""
    from ssdn.params import PipelineOutput as PO
    from test_hip_posterior import _batch, _denoiser
    keys = (PO.IMG_DENOISED, PO.IMG_MU, PO.MODEL_STD_DEV, PO.NOISE_STD_DEV)
    train = [_batch("gauss25", 3, seed=k) for k in range(3)]

    def run(with_ssim):
        d = _denoiser("gauss25", "known", 3)
        data = _eval_batch()
        d.eval()
        with torch.no_grad():
            first = {k: v.clone() for k, v in d.run_pipeline(data).items() if k in keys}
        eng = d._last_engine
        blob = eng.export_plan()
        per = d.accumulate_metrics(data, "eval", with_loss=False, per_sample=True)
        d.accumulate_metrics(data, "keep", with_loss=False)
        if with_ssim:
            d.ssim(data, maps=True)
        d.accumulate_metrics(data, "keep", with_loss=False)
        acc = d.read_metrics("keep")
        assert eng.export_plan() == blob
        with torch.no_grad():
            second = {k: v.clone() for k, v in d.run_pipeline(data).items() if k in keys}
        assert all(torch.equal(first[k], second[k]) for k in keys)
        d.train()
        for k in range(3):
            d.train_step(train[k], lr=3e-4)
            if with_ssim and k < 2:
                d.ssim(train[k])
        torch.cuda.synchronize()
        return first, per, acc, d.flat.detach().clone(), d.adam_m.clone()
    f0, p0, a0, w0, m0 = run(False)
    f1, p1, a1, w1, m1 = run(True)
    assert all(torch.equal(f0[k], f1[k]) for k in keys) and all(torch.equal(p0[k], p1[k]) for k in p0)
    assert a0 == a1 and torch.isfinite(w0).all() and torch.equal(w0, w1) and torch.equal(m0, m1)


def test_cli_eval_ssim_writes_ssims_csv(tmp_path):
    """one `ssdn eval --ssim` over a folder of two images, one of them non-square (loader workers off: their start-up is most of an
    evaluation this small)"""
    from PIL import Image
    from ssdn.__main__ import start_cli
    from ssdn.params import ConfigValue
    from test_hip_posterior import _denoiser
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    for i, (w, h) in enumerate([(40, 24), (32, 32)]):
        a = (R.hash_tensor((h, w, 3), 700 + i, 0, 1).numpy() * 255).astype(np.uint8)
        Image.fromarray(a, mode="RGB").save(imgs / ("im%d.png" % i))
    d = _denoiser("gauss25", "known", 3)
    d.cfg[ConfigValue.DATALOADER_WORKERS] = 0
    torch.save({k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in d.state_dict().items()}, tmp_path / "model.wt")
    from ssdn.eval import DenoiserEvaluator
    results = []
    orig = DenoiserEvaluator.evaluate
    try:
        DenoiserEvaluator.evaluate = lambda self: results.append(orig(self)) or results[-1]
        ev = start_cli(["eval", "-m", str(tmp_path / "model.wt"), "-d", str(imgs), "--runs_dir", str(tmp_path / "runs"), "--batch_size", "2", "--ssim"])
    finally:
        DenoiserEvaluator.evaluate = orig
    names = ["id", "ssim_nsy", "ssim_out", "ssim_mu_out"]
    with open(os.path.join(ev.run_dir_path, "ssims.csv")) as fh:
        assert fh.readline() == ",".join(names) + "\n"
        raw = [ln.strip().split(",") for ln in fh]
    assert [r[0] for r in raw] == ["0000", "0001"] and all(len(r) == 4 for r in raw)
    vals = np.array([[float(v) for v in r[1:]] for r in raw])
    assert np.isfinite(vals).all() and (vals <= 1).all() and (vals[:, 0] < 1).all()
    # the evaluator's engine still holds that batch: Denoiser.ssim against the loader's clean images and extents, to the printed digits
    data = next(iter(ev.testloader))
    again = ev.denoiser.ssim(data)
    for i, r in enumerate(raw):
        assert r[1:] == ["%.6f" % float(again[k][i]) for k in names[1:]]
    with open(os.path.join(ev.run_dir_path, "psnrs.csv")) as fh:
        assert fh.readline() == "id,psnr_nsy,psnr_out,psnr_mu_out\n"
        rows = list(csv.DictReader(fh, fieldnames=["id", "psnr_nsy", "psnr_out", "psnr_mu_out"]))
    assert len(rows) == 2 and all(math.isfinite(float(r["psnr_out"])) for r in rows)
    res = results[0]
    assert abs(res["ssim_out"] - vals[:, 1].mean()) < 2e-6 and abs(res["ssim_mu_out"] - vals[:, 2].mean()) < 2e-6 and "psnr_out" in res
