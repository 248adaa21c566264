"""CPU: training on images that are already noisy -- the host model of SSDN_OP_POOL_PATCH (tests/patch_pool_ref.py: reflection, the eight
transforms, the integer crop origins), ImagePool's packing and cap, the stream's contract on CPU tensors (keys, shapes, dtypes, no CLEAN,
the Noise2Void target, state_dict), every refusal of `--noisy` (the CLI ones through the parser), and the `.training` key.  The GPU side
(the kernel against the model bit for bit, the trainer end to end) is tests/test_hip_patch_pool.py."""
import os

import numpy as np
import pytest
import torch

import patch_pool_ref as R
import ssdn
from ssdn.datasets import DevicePoolStream, ImagePool, NoisyDataset
from ssdn.params import ConfigValue, NoiseAlgorithm, NoiseValue, PipelineOutput

MD = NoisyDataset.Metadata
ALGOS = {"ssdn": NoiseAlgorithm.SELFSUPERVISED_DENOISING, "ssdn_u_only": NoiseAlgorithm.SELFSUPERVISED_DENOISING_MEAN_ONLY,
         "n2v": NoiseAlgorithm.NOISE_TO_VOID}


# ---- 1. the model ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 5, 8])
def test_reflection_is_numpys_reflect_where_numpy_defines_it(n):
    a = np.arange(n) * 3 + 1
    for P in range(n, 2 * n):                          # P - n <= n - 1
        want = np.pad(a, (0, P - n), "reflect")
        assert np.array_equal(a[R.reflect(np.arange(P), n)], want)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_reflection_beyond_one_period_is_the_iterated_pad(n):
    P, a = 8, np.arange(n) * 3 + 1
    want = a.copy()
    while len(want) < P:                               # pad as far as numpy allows, again and again (n = 1: nothing to reflect, the value repeats)
        want = np.pad(want, (0, min(P - len(want), max(len(want) - 1, 1))), "reflect" if len(want) > 1 else "edge")
    assert np.array_equal(a[R.reflect(np.arange(P), n)], want)


def test_the_eight_transforms_are_the_dihedral_group():
    P = 5
    patch = np.arange(P * P, dtype=np.uint8).reshape(1, P, P)            # asymmetric: every element differs
    outs = [R.cut(patch, P, 0, 0, d) for d in range(8)]
    for i in range(8):
        for j in range(i):
            assert not np.array_equal(outs[i], outs[j])
    for d in range(8):
        # out[py, px] = patch[v, u]: bit 2 mirrors the source rows, bit 1 the source columns, bit 0 transposes the result of both
        want = patch[0]
        if d & 4:
            want = np.flip(want, 0)
        if d & 2:
            want = np.flip(want, 1)
        if d & 1:
            want = np.transpose(want)
        assert np.array_equal(outs[d][0], want), d


def test_origins_cover_their_span_and_never_leave_it():
    from philox_ref import _draw
    v = _draw(np.arange(4096), R.NS_CROP, R.SEED, 3)
    for n, P, span in ((12, 8, 5), (8, 8, 1), (3, 8, 1)):
        o = R.origin(v[0], n, P)
        assert o.min() == 0 and o.max() == span - 1 and set(np.unique(o)) == set(range(span))
    assert int(R.origin(0xFFFFFFFF, 12, 8)) == 4 and int(R.origin(0, 12, 8)) == 0
    x0, y0, d = R.draws(7, 9, 40, 8, True, R.SEED, 3)
    w = [int(t) for t in _draw(7, R.NS_CROP, R.SEED, 3)]
    assert (x0, y0, d) == ((w[0] * 33) >> 32, (w[1] * 2) >> 32, w[2] >> 29)
    assert R.draws(7, 9, 40, 8, False, R.SEED, 3)[2] == 0


def test_model_batch_is_cut_of_each_image():
    imgs = R.case_images(3)
    m = R.pool_patch_model(imgs, [6, 2, 6], 8, True, R.SEED, 1, params=np.arange(7) + 0.5)
    for b, i in enumerate([6, 2, 6]):
        x0, y0, d = m["origin"][b]
        assert np.array_equal(m["ref"][b], R.cut(imgs[i], 8, x0, y0, d).astype(np.float32) / np.float32(255))
    assert np.array_equal(m["noisy"], m["ref"]) and m["coords"] is None
    assert np.array_equal(m["param"], np.float32([[6.5] * 3, [2.5] * 3, [6.5] * 3]))
    # Noise2Void: the reference is the unmanipulated patch, the input differs from it at the coordinates only
    m = R.pool_patch_model(imgs, [6, 5], 32, False, R.SEED, 1, n2v_box=8)
    diff = np.argwhere((m["noisy"] != m["ref"]).any(1))
    sel = {(b, int(c1), int(c0)) for b in range(2) for c0, c1 in m["coords"][b]}
    assert m["coords"].shape == (2, 16, 2) and {tuple(t) for t in diff} <= sel and len(diff) > 0
    for b in range(2):
        for (c0, c1), (rx, ry) in zip(m["coords"][b], m["src"][b]):
            assert np.array_equal(m["noisy"][b, :, c1, c0], m["ref"][b, :, ry, rx])


# ---- 2. ImagePool ----------------------------------------------------------------------------------------------------------------------
class _Images(torch.utils.data.Dataset):
    """an untransformed dataset of float [C, rows, cols] tensors, as a folder or HDF5 child hands them out"""
    transform = None

    def __init__(self, arrays):
        self.arrays = arrays

    def __len__(self):
        return len(self.arrays)

    def __getitem__(self, i):
        return torch.from_numpy(self.arrays[i]).float().div_(255.0), i


def _pool(C=3, **kw):
    imgs = R.case_images(C)
    return imgs, ImagePool(_Images(imgs), "cpu", **kw)


def test_pool_packs_back_to_back_without_padding():
    imgs, pool = _pool()
    want_pool, want_off, want_sizes = R.pack(imgs)
    assert pool.n == len(pool) == 7 and pool.channels == 3 and pool.nbytes == want_pool.size
    assert np.array_equal(pool.offsets_host.numpy(), want_off) and pool.offsets.dtype == torch.int64
    assert np.array_equal(pool.offsets_host.numpy(), np.cumsum([0] + [im.size for im in imgs])[:-1])
    assert np.array_equal(pool.sizes.numpy(), want_sizes) and pool.sizes.dtype == torch.int32
    assert np.array_equal(pool.pool.numpy(), want_pool) and pool.pool.dtype == torch.uint8
    assert any(int(o) % 2 for o in want_off)                               # odd offsets: nothing is aligned
    for i, im in enumerate(imgs):
        assert np.array_equal(pool.image(i).numpy(), im)
        assert np.array_equal(pool.upright(i).numpy(), im.transpose(2, 1, 0))


def test_pool_cap_error_names_total_and_cap():
    imgs = R.case_images(3)
    total = sum(im.size for im in imgs)
    with pytest.raises(ValueError) as e:
        ImagePool(_Images(imgs), "cpu", max_bytes=1000)
    assert str(total) in str(e.value) and "1000" in str(e.value) and "pool_gb" in str(e.value)
    assert ImagePool(_Images(imgs), "cpu", max_bytes=total).nbytes == total
    from ssdn.datasets import device_pool
    assert device_pool.DEFAULT_POOL_BYTES == 8 << 30


def test_pool_of_a_folder(tmp_path):
    from PIL import Image
    from ssdn.datasets import UnlabelledImageFolderDataset
    with pytest.raises(RuntimeError, match="Found 0 files"):               # an empty folder: the dataset's own error
        UnlabelledImageFolderDataset(str(tmp_path), channels=3)
    rs = np.random.RandomState(3)
    arrays = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((5, 9), (12, 4))]
    for k, a in enumerate(arrays):
        Image.fromarray(a).save(str(tmp_path / ("im%d.png" % k)))
    ds = UnlabelledImageFolderDataset(str(tmp_path), channels=3)
    pool = ImagePool(ds, "cpu")
    assert pool.files == ds.files and pool.sizes_host.tolist() == [[9, 5], [4, 12]]          # rows run along the picture's x
    for k, a in enumerate(arrays):
        assert np.array_equal(pool.upright(k).numpy(), a)
    with pytest.raises(ValueError, match="cap"):
        ImagePool(ds, "cpu", max_bytes=100)                                 # (refused from the headers alone)
    from ssdn.datasets.transforms import RandomCrop
    with pytest.raises(ValueError, match="untransformed"):
        ImagePool(UnlabelledImageFolderDataset(str(tmp_path), channels=3, transform=RandomCrop(4)), "cpu")


# ---- 3. the stream on CPU tensors ------------------------------------------------------------------------------------------------------
def _stream(algo, P=8, C=3, batches=((0, 1, 2, 3, 3), (4, 5, 6, 6, 0)), **kw):
    imgs, pool = _pool(C)
    return imgs, pool, DevicePoolStream(pool, [list(b) for b in batches], ALGOS[algo], "gauss25", P, seed=11, **kw)


@pytest.mark.parametrize("algo", ["ssdn", "ssdn_u_only", "n2v"])
@pytest.mark.parametrize("C", [1, 3])
def test_cpu_stream_contract(algo, C):
    imgs, pool, st = _stream(algo, C=C, augment=True)
    st.keep_origin = True
    assert len(st) == 2
    it = iter(st)
    for idx in ((0, 1, 2, 3, 3), (4, 5, 6, 6, 0)):
        inp, ref, meta = next(it)
        B = 5
        assert MD.CLEAN not in meta
        want = {MD.INDEXES, MD.IMAGE_SHAPE, MD.INPUT_NOISE_VALUES, MD.REFERENCE_NOISE_VALUES} | ({MD.MASK_COORDS} if algo == "n2v" else set())
        assert set(meta) == want
        assert inp.shape == (B, C, 8, 8) and inp.dtype == torch.float32
        assert meta[MD.INDEXES].tolist() == list(idx) and meta[MD.INDEXES].dtype == torch.int64
        assert meta[MD.IMAGE_SHAPE].tolist() == [[C, 8, 8]] * B
        for k in (MD.INPUT_NOISE_VALUES, MD.REFERENCE_NOISE_VALUES):
            assert meta[k].shape == (B, 1, 1, 1) and meta[k].dtype == torch.float32
        assert torch.all(meta[MD.INPUT_NOISE_VALUES] == np.float32(25 / 255.0)) and meta[MD.INPUT_NOISE_VALUES]._ssdn_const
        # the unmanipulated patch is the model's cut at the origin the stream drew
        plain = np.stack([R.cut(imgs[i], 8, *[int(v) for v in st.last_origin[b]]) for b, i in enumerate(idx)]).astype(np.float32) / np.float32(255)
        assert set(st.last_origin[:, 2].tolist()) <= set(range(8))
        if algo == "ssdn":
            assert ref.shape == (B, 0) and torch.all(meta[MD.REFERENCE_NOISE_VALUES] == 0)
            assert np.array_equal(inp.numpy(), plain)
        elif algo == "ssdn_u_only":
            assert ref is inp and meta[MD.REFERENCE_NOISE_VALUES] is meta[MD.INPUT_NOISE_VALUES]
            assert np.array_equal(inp.numpy(), plain)
        else:
            co = meta[MD.MASK_COORDS]
            assert co.shape == (B, 1, 2) and co.dtype == torch.int64
            assert np.array_equal(ref.numpy(), plain)                   # the textbook Noise2Void target
            changed = {tuple(t) for t in np.argwhere((inp.numpy() != plain).any(1))}
            assert changed <= {(b, int(co[b, 0, 1]), int(co[b, 0, 0])) for b in range(B)}
    assert next(it, None) is None and st.state_dict() == {"seed": 11, "calls": 2}


def test_cpu_stream_per_image_parameters_and_state_dict():
    imgs, pool = _pool(3)
    with pytest.raises(ValueError, match="set_params"):
        DevicePoolStream(pool, [[0]], ALGOS["ssdn"], "gauss25", 8, per_image=True)
    with pytest.raises(ValueError, match="7 images"):
        pool.set_params([1.0, 2.0])
    pool.set_params(np.arange(7) * 0.01 + 0.02)
    batches = [[6, 6, 1], [2, 0, 5], [3, 4, 4]]
    st = DevicePoolStream(pool, batches, ALGOS["ssdn"], "gauss25", 8, augment=True, per_image=True, seed=5, rank=2)
    it = iter(st)
    first = next(it)
    npv = first[2][MD.INPUT_NOISE_VALUES]
    assert npv.shape == (3, 3, 1, 1) and npv._ssdn_per_sample
    assert torch.equal(npv[:, :, 0, 0], pool.params_host[[6, 6, 1]].view(3, 1).expand(3, 3))
    sd = st.state_dict()
    assert sd == {"seed": 5, "calls": 1} and st.seed == 7
    rest = [b[0].clone() for b in it]
    # a second stream continued from the state dict yields the same remaining minibatches
    st2 = DevicePoolStream(pool, batches[1:], ALGOS["ssdn"], "gauss25", 8, augment=True, per_image=True, seed=99, rank=2)
    st2.load_state_dict(sd)
    assert st2.state_dict() == sd and st2.seed == 7
    # (the CPU generator is not part of the state: compare what does not depend on it -- with patches as large as the images nothing is drawn)
    big = DevicePoolStream(pool, [[3]], ALGOS["ssdn"], "gauss25", 8, seed=1)
    assert np.array_equal(next(iter(big))[0][0].numpy(), imgs[3].astype(np.float32) / np.float32(255))
    assert len(rest) == 2 and st.state_dict()["calls"] == 3
    with pytest.raises(IndexError):
        st.prepare([0, 7])
    with pytest.raises(IndexError):
        st.prepare([-1])


def test_stream_refuses_pipelines_that_need_a_clean_image():
    _, pool = _pool(3)
    for algo in (NoiseAlgorithm.NOISE_TO_CLEAN, NoiseAlgorithm.NOISE_TO_NOISE):
        with pytest.raises(ValueError, match="clean image or a second realisation"):
            DevicePoolStream(pool, [[0]], algo, "gauss25", 8)


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------
def _cfg(algo="ssdn", style="gauss25", value="known", patch=32):
    cfg = ssdn.cfg.base()
    cfg[ConfigValue.ALGORITHM] = NoiseAlgorithm(algo)
    cfg[ConfigValue.NOISE_STYLE] = style
    if value is not None:
        cfg[ConfigValue.NOISE_VALUE] = NoiseValue(value)
    cfg[ConfigValue.TRAIN_PATCH_SIZE] = patch
    return cfg


REFUSALS = [
    (dict(algo="n2c", value=None), "style", {}, "clean image or a second realisation"),
    (dict(algo="n2n", value=None), "style", {}, "clean image or a second realisation"),
    (dict(style="gauss5_50"), "style", {}, "--noisy auto"),
    (dict(style="impulse50"), "auto", {}, "no noise-level estimator"),
    (dict(algo="n2v", value=None), "auto", {}, "reads none"),
    (dict(algo="ssdn_u_only", value=None), "auto", {}, "reads none"),
    (dict(value="const"), "auto", {}, "reads none"),
    (dict(value="var"), "auto", {}, "reads none"),
    (dict(), None, dict(augment=True), "needs --noisy"),
    (dict(), None, dict(pool_bytes=1 << 30), "needs --noisy"),
    (dict(patch=40), "style", {}, "multiple of 32"),
    (dict(), "sometimes", {}, "one of style, auto"),
]


@pytest.mark.parametrize("cfg_kw, noisy, kw, text", REFUSALS)
def test_check_noisy_refuses_with_advice(cfg_kw, noisy, kw, text):
    from ssdn.train import check_noisy
    with pytest.raises(ValueError) as e:
        check_noisy(_cfg(**cfg_kw), noisy, **kw)
    assert text in str(e.value)


def test_check_noisy_accepts_what_works():
    from ssdn.train import check_noisy
    check_noisy(_cfg(), None)
    check_noisy(_cfg(), "style", augment=True, pool_bytes=1 << 20)
    check_noisy(_cfg(), "auto")
    check_noisy(_cfg(style="poisson30"), "auto")
    check_noisy(_cfg(style="gauss5_50", value="const"), "style")            # a ranged style whose parameter nobody reads
    check_noisy(_cfg(algo="n2v", value=None, style="gauss5_50"), "style")
    check_noisy(_cfg(algo="ssdn_u_only", value=None), "style")


CLI_BASE = ["train", "start", "-t", "nowhere", "-i", "16", "--patch_size", "32"]
CLI_REFUSALS = [
    (["-a", "n2c", "-n", "gauss25", "--noisy"], "clean image or a second realisation"),
    (["-a", "n2n", "-n", "gauss25", "--noisy", "style"], "clean image or a second realisation"),
    (["-a", "ssdn", "--noise_value", "known", "-n", "gauss5_50", "--noisy"], "--noisy auto"),
    (["-a", "ssdn", "--noise_value", "known", "-n", "impulse50", "--noisy", "auto"], "no noise-level estimator"),
    (["-a", "n2v", "-n", "gauss25", "--noisy", "auto"], "reads none"),
    (["-a", "ssdn", "--noise_value", "const", "-n", "gauss25", "--noisy", "auto"], "reads none"),
    (["-a", "ssdn", "--noise_value", "known", "-n", "gauss25", "--augment"], "needs --noisy"),
    (["-a", "ssdn", "--noise_value", "known", "-n", "gauss25", "--pool_gb", "2"], "needs --noisy"),
    (["-a", "ssdn", "--noise_value", "known", "-n", "gauss25", "--noisy", "--patch_size", "40"], "multiple of 32"),
    (["-a", "ssdn", "--noise_value", "known", "-n", "gauss25", "--noisy", "--pool_gb", "0"], "must be positive"),
    (["-a", "ssdn", "--noise_value", "known", "-n", "gauss25", "--noisy", "maybe"], "invalid choice"),
]


@pytest.mark.parametrize("extra, text", CLI_REFUSALS)
def test_cli_refusals_go_through_the_parser(extra, text, capsys, tmp_path):
    from ssdn.cli.cli import start
    with pytest.raises(SystemExit) as e:
        start(CLI_BASE + ["--runs_dir", str(tmp_path)] + extra)
    assert e.value.code == 2
    assert text in capsys.readouterr().err
    assert not os.listdir(str(tmp_path))                                   # refused before anything was written


def test_cli_flags_parse():
    from ssdn.cli.cli import build_parser
    p, _ = build_parser()
    base = CLI_BASE + ["-a", "ssdn", "--noise_value", "known", "-n", "gauss25"]
    a = p.parse_args(base)
    assert a.noisy is None and a.augment is False and a.pool_gb is None
    a = p.parse_args(base + ["--noisy"])
    assert a.noisy == "style"
    a = p.parse_args(base + ["--noisy", "auto", "--augment", "--pool_gb", "0.5"])
    assert a.noisy == "auto" and a.augment is True and a.pool_gb == 0.5
    with pytest.raises(SystemExit):                                        # resume continues what the run was started with
        p.parse_args(["train", "resume", "some/run", "--noisy"])


# ---- 5. the trainer without a GPU: a stub target over the CPU stream --------------------------------------------------------------------
def _stub(cfg):
    from ssdn.denoiser import Denoiser

    class Stub(Denoiser):
        def __init__(self, cfg):
            super().__init__(cfg, device="cpu")
            self.batches = []

        def train_step(self, data, lr, exchange=None):
            inp, meta = data[NoisyDataset.INPUT], data[NoisyDataset.METADATA]
            self.batches.append((meta[MD.INDEXES].tolist(), inp.clone(), set(meta)))
            n = inp.shape[0]
            return {PipelineOutput.INPUTS: data, PipelineOutput.LOSS: torch.ones(n, 1), PipelineOutput.IMG_DENOISED: inp.clone(),
                    PipelineOutput.IMG_MU: inp.clone(), PipelineOutput.NOISE_STD_DEV: torch.ones(n, 1, 1),
                    PipelineOutput.MODEL_STD_DEV: torch.ones(n, inp.shape[2], inp.shape[3])}
    return Stub(cfg)


def _train(tmp_path, folder, runs, noisy, iters=12):
    from ssdn.train import DenoiserTrainer
    cfg = _cfg()
    cfg[ConfigValue.TRAIN_ITERATIONS], cfg[ConfigValue.TRAIN_MINIBATCH_SIZE] = iters, 4
    cfg[ConfigValue.TRAIN_DATA_PATH], cfg[ConfigValue.DATALOADER_WORKERS] = folder, 0
    cfg[ConfigValue.PRINT_INTERVAL], cfg[ConfigValue.EVAL_INTERVAL], cfg[ConfigValue.SNAPSHOT_INTERVAL] = 4, 10 ** 9, 8
    torch.manual_seed(3)
    tr = DenoiserTrainer(cfg, runs_dir=str(tmp_path / runs))
    tr.noisy, tr.augment = noisy, bool(noisy)
    tr.device_data = False
    tr.denoiser = _stub(tr.cfg)
    tr.init_state()
    tr.train()
    return tr


def test_trainer_on_noisy_images_without_a_gpu(tmp_path, monkeypatch):
    from PIL import Image
    from ssdn.train import resume_run
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    folder = str(tmp_path / "noisy")
    os.makedirs(folder)
    rs = np.random.RandomState(1)
    arrays = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in ((40, 48), (33, 70), (20, 36), (64, 32), (32, 32), (50, 41))]
    for k, a in enumerate(arrays):
        Image.fromarray(a).save(os.path.join(folder, "im%d.png" % k))
    tr = _train(tmp_path, folder, "runs", "style")
    assert isinstance(tr.trainloader, DevicePoolStream) and tr.trainloader.augment
    d = tr.denoiser
    assert len(d.batches) == 3 and all(len(b[0]) == 4 and b[1].shape == (4, 3, 32, 32) for b in d.batches)
    assert all(MD.CLEAN not in b[2] for b in d.batches)
    # every patch is made of bytes of its own image (the 20 x 36 one is smaller than the patch: reflected, so still its own bytes)
    for idx, inp, _ in d.batches:
        for b, i in enumerate(idx):
            vals = set(np.unique(np.round(inp[b].numpy() * 255).astype(np.uint8)))
            assert vals <= set(np.unique(arrays[i]))
    log = open(os.path.join(tr.run_dir_path, "log.txt")).read()
    lines = [ln for ln in log.splitlines() if "TRAIN |" in ln]
    assert len(lines) >= 3 and all("psnr" not in ln for ln in lines) and any("loss=" in ln for ln in lines)
    assert "psnr" not in open(os.path.join(tr.run_dir_path, "scalars.csv")).read()
    # `.training`: the extra key only when the mode is on; resume restores it
    sd = torch.load(os.path.join(tr.run_dir_path, "training", "model_00000012.training"), map_location="cpu", weights_only=False)
    assert sd["noisy"] == {"mode": "style", "augment": True, "pool_bytes": None} and sd["device_stream"]["calls"] == 3
    tr0 = _train(tmp_path, folder, "runs0", None)
    sd0 = torch.load(os.path.join(tr0.run_dir_path, "training", "model_00000012.training"), map_location="cpu", weights_only=False)
    assert "noisy" not in sd0 and set(sd) - set(sd0) == {"noisy", "device_stream"}
    r = resume_run(tr.run_dir_path, 8)
    assert r.noisy == "style" and r.augment is True and r.pool_bytes is None and r._stream_state["calls"] == 2
    r0 = resume_run(tr0.run_dir_path)
    assert r0.noisy is None and r0.augment is False
    # a trainer whose patch size the network cannot take is refused in this mode
    from ssdn.train import DenoiserTrainer
    bad = DenoiserTrainer(_cfg(patch=40), runs_dir=str(tmp_path / "runs2"))
    bad.noisy = "style"
    bad.cfg[ConfigValue.TRAIN_DATA_PATH] = folder
    with pytest.raises(ValueError, match="multiple of 32"):
        bad.train_data()
