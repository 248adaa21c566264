"""GPU: training on images that are already noisy.  SSDN_OP_POOL_PATCH (csrc/patch_pool.hip) against the numpy model tests/patch_pool_ref.py
bit for bit -- the model is integer arithmetic plus one correctly rounded division, so there is no tolerance and nothing is excluded --,
its 64-bit addressing, the launch's refusals; DevicePoolStream feeding `Denoiser.train_step` unchanged; the metrics of a batch without a
clean image; the per-image parameters of `--noisy auto`; and `ssdn train start --noisy` end to end with a bit-identical resume."""
import ctypes as C
import glob
import math
import os
import shutil

import numpy as np
import pytest
import torch

import patch_pool_ref as R
from head_ops import DEV, P, run_one

pytestmark = pytest.mark.gpu
GUARD = 64                      # elements in front of and behind every output
BOX = 8                         # ssdn.utils.n2v_ups._box_size()


class _Out:
    """an output between guards: poisoned (NaN; integers: a sentinel) before the launch"""

    def __init__(self, shape, dtype):
        self.n, self.shape = int(np.prod(shape)), shape
        self.poison = float("nan") if dtype.is_floating_point else -0x5A5A5A5A
        self.guard = 12345.0 if dtype.is_floating_point else 0x77777777
        self.buf = torch.full((self.n + 2 * GUARD,), self.guard, dtype=dtype, device=DEV)
        self.buf[GUARD:GUARD + self.n] = self.poison

    @property
    def ptr(self):
        return self.buf.data_ptr() + GUARD * self.buf.element_size()

    def read(self):
        h = self.buf.cpu().numpy()
        assert (h[:GUARD] == self.guard).all() and (h[GUARD + self.n:] == self.guard).all(), "guard overwritten"
        v = h[GUARD:GUARD + self.n].reshape(self.shape)
        assert not (np.isnan(v).any() if v.dtype.kind == "f" else (v == self.poison).any()), "an element was not written"
        return v


def _device_pool(images, params=None, base=0, pool=None):
    hp, off, sizes = R.pack(images)
    d = dict(pool=torch.from_numpy(hp).to(DEV) if pool is None else pool, offsets=torch.from_numpy(off + base).to(DEV),
             sizes=torch.from_numpy(sizes).to(DEV).contiguous(), N=len(images),
             params=torch.tensor(params, dtype=torch.float32, device=DEV) if params is not None else None)
    return d


def pool_patch_op(dp, index, Cn, Pn, augment, seed, offset, n2v_box=0):
    from ssdn.hip import lib as L
    B = len(index)
    idx = torch.tensor(index, dtype=torch.int32, device=DEV)
    cells = (Pn // n2v_box) ** 2 if n2v_box else 0
    noisy, ref = _Out((B, Cn, Pn, Pn), torch.float32), _Out((B, Cn, Pn, Pn), torch.float32)
    coords = _Out((B, cells, 2), torch.int64) if n2v_box else None
    par, org = _Out((B, Cn), torch.float32), _Out((B, 3), torch.int32)
    a = L.PoolPatchArgs(P(dp["pool"]), P(dp["offsets"]), P(dp["sizes"]), P(dp["params"]), P(idx), noisy.ptr, ref.ptr,
                        coords.ptr if coords else None, par.ptr if dp["params"] is not None else None, org.ptr,
                        dp["N"], B, Cn, Pn, int(augment), n2v_box, 2, seed, offset)
    run_one("pool_patch", a)
    return dict(noisy=noisy.read(), ref=ref.read(), coords=coords.read() if coords else None,
                param=par.read() if dp["params"] is not None else None, origin=org.read())


# ---- 1. the op against the model, bit for bit --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n2v_box", [0, BOX])
@pytest.mark.parametrize("augment", [False, True])
@pytest.mark.parametrize("Pn", [8, 32])
@pytest.mark.parametrize("Cn", [1, 3])
def test_op_against_the_numpy_model_bit_for_bit(Cn, Pn, augment, n2v_box):
    images = R.case_images(Cn)
    params = [0.01 * (i + 1) + 1 / 3 for i in range(len(images))]
    dp = _device_pool(images, params)
    assert any(int(o) % 2 for o in dp["offsets"].cpu())
    seen, transforms = set(), set()
    for index, offset in zip(R.INDEXES, (R.OFFSETS[0], R.OFFSETS[1], R.OFFSETS[0])):
        got = pool_patch_op(dp, index, Cn, Pn, augment, R.SEED, offset, n2v_box)
        m = R.pool_patch_model(images, index, Pn, augment, R.SEED, offset, params=params, n2v_box=n2v_box)
        assert np.array_equal(got["origin"], m["origin"])
        assert got["noisy"].dtype == np.float32 and np.array_equal(got["noisy"], m["noisy"])
        assert np.array_equal(got["ref"], m["ref"])
        assert np.array_equal(got["param"], m["param"])
        if n2v_box:
            assert np.array_equal(got["coords"], m["coords"])
            assert (m["noisy"] != m["ref"]).any()
        else:
            assert np.array_equal(got["noisy"], got["ref"])
        seen |= set(index)
        transforms |= set(m["origin"][:, 2].tolist())
    assert seen == set(range(len(images)))
    assert (len(transforms) >= 4) if augment else (transforms == {0})
    # the same sample number under two offsets draws differently (image 6 is larger than either patch)
    a = R.pool_patch_model(images, [6] * 5, Pn, True, R.SEED, R.OFFSETS[0])["origin"]
    b = R.pool_patch_model(images, [6] * 5, Pn, True, R.SEED, R.OFFSETS[1])["origin"]
    assert not np.array_equal(a, b)


# ---- 2. 64-bit addressing ----------------------------------------------------------------------------------------------------------------
def test_an_image_beyond_two_gib_is_addressed_with_64_bits():
    free, _ = torch.cuda.mem_get_info()
    if free < 4 << 30:
        pytest.skip("less than 4 GiB of device memory free")
    Cn, base = 3, 2 ** 31 + 5
    img = np.random.RandomState(9).randint(0, 256, (Cn, 9, 8)).astype(np.uint8)
    pool = torch.empty(base + img.size, dtype=torch.uint8, device=DEV)
    pool[base:] = torch.from_numpy(img.reshape(-1)).to(DEV)                  # only those bytes are filled
    dp = _device_pool([img], base=base, pool=pool)
    got = pool_patch_op(dp, [0, 0, 0], Cn, 8, True, R.SEED, 4)
    m = R.pool_patch_model([img], [0, 0, 0], 8, True, R.SEED, 4)
    assert np.array_equal(got["origin"], m["origin"]) and np.array_equal(got["noisy"], m["noisy"]) and np.array_equal(got["ref"], m["ref"])
    del pool, dp
    torch.cuda.empty_cache()


# ---- 3. the launch's refusals ------------------------------------------------------------------------------------------------------------
def test_launch_refusals_launch_nothing():
    from ssdn.hip import lib as L
    images = R.case_images(1)
    dp = _device_pool(images, [1.0] * 7)
    idx = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    out = _Out((2, 1, 8, 8), torch.float32)
    co = _Out((2, 1, 2), torch.int64)

    def args(**kw):
        a = L.PoolPatchArgs(P(dp["pool"]), P(dp["offsets"]), P(dp["sizes"]), P(dp["params"]), P(idx), out.ptr, None, None, None, None,
                            7, 2, 1, 8, 0, 0, 2, 1, 0)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(text, **kw):
        a = args(**kw)
        rec = (L.OpRec * 1)()
        rec[0].type, rec[0].lane, rec[0].args = L.OP["pool_patch"], 0, C.cast(C.pointer(a), C.c_void_p)
        rc = L.load().ssdn_run_ops(rec, 1, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        msg = L.load().ssdn_last_error().decode()
        assert rc != 0 and "pool_patch: " in msg and text in msg, (rc, msg)          # (the executor prefixes the op's position in the list)
    for name in ("pool", "offsets", "sizes", "index", "noisy32"):
        refused("are required", **{name: None})
    for name in ("N", "B", "C", "P"):
        refused("empty shape", **{name: 0})
        refused("empty shape", **{name: -1})
    refused("32-bit indexing", B=1 << 15, P=256)                               # B C P P = 2^31
    refused("params table", params=None, param_out=out.ptr)
    refused("coords output", n2v_box=8)
    refused("multiple of n2v_box", n2v_box=3, coords=co.ptr)
    refused("n2v_radius must be >= 1", n2v_box=8, coords=co.ptr, n2v_radius=0)
    refused("larger than 1 pixel", n2v_box=1, coords=co.ptr, P=1)
    refused("at most P", n2v_box=8, coords=co.ptr, n2v_radius=9)
    torch.cuda.synchronize()
    h = out.buf.cpu().numpy()
    assert np.isnan(h[GUARD:GUARD + out.n]).all()                             # nothing was launched
    run_one("pool_patch", args())                                             # ... and the unmodified arguments are accepted
    out.read()


# ---- 4. / 5. the stream feeds the step unchanged; metrics without a clean image ------------------------------------------------------------
class _Images(torch.utils.data.Dataset):
    transform = None

    def __init__(self, arrays):
        self.arrays = arrays

    def __len__(self):
        return len(self.arrays)

    def __getitem__(self, i):
        return torch.from_numpy(self.arrays[i]).float().div_(255.0), i


def _denoiser(alg="ssdn", style="gauss25", mode="known"):
    from test_hip_denoiser import make_denoiser
    torch.manual_seed(77)
    return make_denoiser(alg, style, mode, 3)


@pytest.fixture(scope="module")
def stream_steps():
    from ssdn.datasets import DevicePoolStream, ImagePool, NoisyDataset
    from ssdn.datasets.noise_wrapper import NULL_IMAGE
    from ssdn.params import NoiseAlgorithm
    MD = NoisyDataset.Metadata
    arrays = [np.random.RandomState(40 + i).randint(0, 256, (3, 32, 32)).astype(np.uint8) for i in range(5)]
    pool = ImagePool(_Images(arrays), DEV)
    batches = [[0, 3, 3, 1], [4, 2, 0, 1]]
    d1 = _denoiser()
    d2 = _denoiser()
    d2.load_state_dict(d1.state_dict())
    d2.mark_dirty()
    assert torch.equal(d1.flat, d2.flat)
    st = DevicePoolStream(pool, batches, NoiseAlgorithm.SELFSUPERVISED_DENOISING, "gauss25", 32, seed=3).attach(d1)
    d1.train()
    d2.train()
    seen = []
    for data in st:
        seen.append((data[0].clone(), data[2]))
        d1.train_step(data, 1e-3, metrics=True)
    torch.cuda.synchronize()
    m1 = d1.read_metrics("train")
    attached = data[0].data_ptr() == d1.input_buffer(4, 32, 32).data_ptr()
    for inp, meta in seen:                       # hand-built batches of the same tensors, with a CLEAN tensor supplied
        hand = {MD.INPUT_NOISE_VALUES: torch.full((4, 1, 1, 1), 25 / 255.0, device=DEV), MD.CLEAN: inp.clone(),
                MD.IMAGE_SHAPE: torch.tensor([3, 32, 32]).repeat(4, 1), MD.INDEXES: meta[MD.INDEXES]}
        d2.train_step([inp.clone(), torch.stack([NULL_IMAGE] * 4).to(DEV), hand], 1e-3, metrics=True)
    torch.cuda.synchronize()
    return dict(arrays=arrays, batches=batches, seen=seen, d1=d1, d2=d2, m1=m1, m2=d2.read_metrics("train"), attached=attached)


def test_stream_input_is_the_bytes_of_the_indexed_images(stream_steps):
    from ssdn.datasets import NoisyDataset
    MD = NoisyDataset.Metadata
    s = stream_steps
    for (inp, meta), idx in zip(s["seen"], s["batches"]):
        want = np.stack([s["arrays"][i] for i in idx]).astype(np.float32) / np.float32(255)
        assert np.array_equal(inp.cpu().numpy(), want)
        assert MD.CLEAN not in meta and meta[MD.INDEXES].tolist() == idx
        assert torch.equal(meta[MD.INPUT_NOISE_VALUES].cpu(), torch.full((4, 1, 1, 1), 25 / 255.0))
    assert s["attached"]                          # the second minibatch was written straight into the engine's input buffer


def test_two_steps_from_the_stream_equal_two_steps_on_hand_built_batches(stream_steps):
    assert torch.equal(stream_steps["d1"].flat, stream_steps["d2"].flat)
    assert stream_steps["d1"].adam_steps == stream_steps["d2"].adam_steps == 2


def test_metrics_without_a_clean_image(stream_steps):
    from ssdn.params import PipelineOutput
    m1, m2 = stream_steps["m1"], stream_steps["m2"]
    assert set(m1) == {"loss", PipelineOutput.NOISE_STD_DEV.value, PipelineOutput.MODEL_STD_DEV.value}
    assert {"psnr_out", "psnr_mu_out"} <= set(m2)
    assert m1["loss"][1] == 8 and math.isfinite(m1["loss"][0])
    for k in m1:
        assert m1[k] == m2[k], k                  # bit-equal sums, equal counts
    d = stream_steps["d1"]
    data = [stream_steps["seen"][-1][0], None, stream_steps["seen"][-1][1]]
    with pytest.raises(ValueError, match="no clean image"):
        d.ssim(data)
    with pytest.raises(ValueError, match="no clean image"):
        d.calibration(data)


# ---- 6. auto -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gauss", "poisson"])
def test_auto_parameters_are_estimate_noise_per_image(kind):
    import noise_est_ref as NE
    from ssdn.datasets import DevicePoolStream, ImagePool, NoisyDataset
    from ssdn.params import NoiseAlgorithm
    MD = NoisyDataset.Metadata
    upright = NE.make_images([(64, 64), (63, 65), (64, 64)], 3, seed=5)
    d = _denoiser(style="gauss25" if kind == "gauss" else "poisson30")
    pool = ImagePool(_Images([np.ascontiguousarray(u.transpose(2, 1, 0)) for u in upright]), DEV)
    pool.estimate_params(d, kind)
    est = d.estimate_noise(upright, kind=kind)
    want = np.array([e["noise_param"] for e in est], dtype=np.float32)
    assert np.isfinite(want).all() and np.array_equal(pool.params.cpu().numpy(), want)
    key = "sigma" if kind == "gauss" else "lambda"          # sigma in byte units / 255, lambda as it is (one fp32 rounding apart at most)
    f64 = np.array([e[key] / 255.0 if kind == "gauss" else e[key] for e in est])
    assert bool((np.abs(want - f64) <= 2.0 ** -23 * np.abs(f64)).all()) and len(set(want.tolist())) == 3
    index = [2, 0, 2, 1]
    st = DevicePoolStream(pool, [index], NoiseAlgorithm.SELFSUPERVISED_DENOISING, "gauss25" if kind == "gauss" else "poisson30", 32,
                          per_image=True, seed=1)
    data = next(iter(st))
    npv = data[2][MD.INPUT_NOISE_VALUES]
    assert npv.shape == (4, 3, 1, 1) and np.array_equal(npv.cpu().numpy()[:, :, 0, 0], np.repeat(want[index][:, None], 3, 1))
    d.train()
    out = d.train_step(data, 1e-4)
    torch.cuda.synchronize()
    assert np.array_equal(d._last_train_engine.noise_param.cpu().numpy(), want[index])       # each sample trained with its own image's value
    from ssdn.params import PipelineOutput
    assert torch.isfinite(out[PipelineOutput.LOSS]).all()


# ---- 7. / 8. the trainer end to end, and a bit-identical resume ----------------------------------------------------------------------------
def _noisy_folder(path):
    from PIL import Image
    os.makedirs(path)
    rs = np.random.RandomState(2)
    for k, (h, w) in enumerate(((40, 56), (33, 70), (20, 36), (64, 35), (48, 48), (50, 41))):      # one smaller than the patch
        yy, xx = np.mgrid[0:h, 0:w]
        base = 0.5 + 0.3 * np.sin(xx / (5.0 + k)) * np.cos(yy / 7.0)
        img = np.stack([base, 1 - base, np.roll(base, 3, 1)], -1) + rs.randn(h, w, 3) * (25 / 255.0)
        Image.fromarray(np.uint8(np.clip(img, 0, 1) * 255)).save(os.path.join(path, "im%d.png" % k))


@pytest.fixture(scope="module")
def noisy_run(tmp_path_factory):
    from ssdn.__main__ import start_cli
    root = tmp_path_factory.mktemp("noisy_run")
    data = str(root / "photos")
    _noisy_folder(data)
    torch.manual_seed(20261021)
    tr = start_cli(["train", "start", "--noisy", "-a", "ssdn", "--noise_value", "known", "-n", "gauss25", "-t", data, "-i", "16",
                    "--train_batch_size", "4", "--patch_size", "32", "--print_interval", "4", "--checkpoint_interval", "8",
                    "--runs_dir", str(root / "runs")])
    return root, tr


def test_cli_trains_on_a_folder_of_noisy_images(noisy_run):
    from ssdn.datasets import DevicePoolStream
    from ssdn.params import StateValue
    from test_hip_trainer import _scalars
    _, tr = noisy_run
    run = tr.run_dir_path
    assert isinstance(tr.trainloader, DevicePoolStream) and tr.state[StateValue.ITERATION] == 16
    assert len(glob.glob(os.path.join(run, "final-*.wt"))) == 1
    log = open(os.path.join(run, "log.txt")).read()
    lines = [ln for ln in log.splitlines() if "TRAIN |" in ln]
    assert "TRAINING FINISHED" in log and len(lines) >= 4 and all("psnr" not in ln for ln in lines)
    sc = _scalars(run)
    assert [s for s, _ in sc["train/loss"]] == [4, 8, 12, 16] and all(np.isfinite(v) for _, v in sc["train/loss"])
    assert not any("psnr" in k for k in sc)
    sd = torch.load(os.path.join(run, "training", "model_00000016.training"), map_location="cpu", weights_only=False)
    assert sd["noisy"]["mode"] == "style" and sd["device_stream"]["calls"] == 4


def test_resumed_noisy_run_is_bit_identical_to_the_uninterrupted_one(noisy_run):
    from ssdn.params import StateValue
    from ssdn.train import resume_run
    root, tr = noisy_run
    run = tr.run_dir_path
    copy = str(root / "runs_resumed" / os.path.basename(run))
    shutil.copytree(run, copy)
    for p in glob.glob(os.path.join(copy, "final-*.wt")) + [os.path.join(copy, "training", "model_00000016.training")]:
        os.remove(p)
    r = resume_run(copy, iteration=8)
    assert r.noisy == "style" and r.state[StateValue.ITERATION] == 8
    r.train()
    assert r.state[StateValue.ITERATION] == 16
    a = torch.load(glob.glob(os.path.join(run, "final-*.wt"))[0], map_location="cpu", weights_only=False)
    b = torch.load(glob.glob(os.path.join(copy, "final-*.wt"))[0], map_location="cpu", weights_only=False)

    def tensors(o, pre=""):
        if torch.is_tensor(o):
            yield pre, o
        elif isinstance(o, dict):
            for k in o:
                yield from tensors(o[k], pre + "/" + str(k))
    ta, tb = dict(tensors(a)), dict(tensors(b))
    assert ta.keys() == tb.keys() and len(ta) > 10
    for k in ta:
        assert torch.equal(ta[k], tb[k]), k
    assert not torch.equal(tr.denoiser.flat.cpu(), torch.zeros_like(tr.denoiser.flat.cpu()))


# ---- 9. n2v and ssdn_u_only ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", ["n2v", "ssdn_u_only"])
def test_the_other_two_pipelines_step_from_the_pool(alg):
    from ssdn.datasets import DevicePoolStream, ImagePool, NoisyDataset
    from ssdn.params import NoiseAlgorithm, PipelineOutput
    MD = NoisyDataset.Metadata
    arrays = [np.random.RandomState(60 + i).randint(0, 256, (3, r, c)).astype(np.uint8) for i, (r, c) in enumerate(((40, 33), (32, 64), (20, 50)))]
    pool = ImagePool(_Images(arrays), DEV)
    d = _denoiser(alg)
    d.train()
    st = DevicePoolStream(pool, [[0, 1, 2, 1], [2, 2, 0, 1]], NoiseAlgorithm(alg), "gauss25", 32, augment=True, seed=8).attach(d)
    n = 0
    for data in st:
        if alg == "n2v":
            assert data[2][MD.MASK_COORDS].shape == (4, 16, 2) and data[1].shape == data[0].shape
            changed = (data[0] != data[1]).any(1).sum().item()
            assert 0 < changed <= 4 * 16
        out = d.train_step(data, 1e-4, metrics=True)
        torch.cuda.synchronize()
        assert torch.isfinite(out[PipelineOutput.LOSS]).all()
        n += 1
    assert n == 2 and d.adam_steps == 2
    m = d.read_metrics("train")
    assert "loss" in m and not any(k.startswith("psnr") for k in m) and math.isfinite(m["loss"][0])
