"""Training on a folder of noisy images -- a measurement aid, not a test.

Generates a folder of synthetic noisy PNGs in a temporary directory and reports, as one JSON line each:
  (a) pool_stream:  patches/s of DevicePoolStream alone (one SSDN_OP_POOL_PATCH launch per minibatch, nothing trained)
  (b) train_pool:   images/s of the training loop of `ssdn train --noisy` (DenoiserTrainer.train_data -> Denoiser.train_step with metrics)
  (c) train_folder: images/s of the same loop over the route such a folder took before: DevicePatchStream over
                    UnlabelledImageFolderDataset with the configured DataLoader workers, noise synthesis on
and the sha256 of the library that ran.  (b) and (c) run in this one process on the same device, one after the other.

--depth both measures something else: the same pictures once as an 8-bit pool (SSDN_OP_POOL_PATCH) and once widened
to uint16 at white = 255 (SSDN_OP_POOL_PATCH16: the same values, so the same training step), ImagePool.from_images -> DevicePoolStream ->
Denoiser.train_step(metrics=True), `--rounds` runs of each alternating in this one process: one JSON line per run, then the medians and
their ratio.

usage: python tools/patch_pool_bench.py [--images 48] [--height 256] [--width 384] [--batch 32] [--patch 64] [--steps 200] [--warmup 20]
                                        [--folder_steps 40] [--workers 4] [--depth both [--rounds 3]] [--out FILE]"""
import argparse
import hashlib
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "selfsupervised-denoising_amd"), ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import ssdn  # noqa: E402
from ssdn.params import ConfigValue, NoiseAlgorithm, NoiseValue  # noqa: E402


def make_pictures(n, h, w, sigma=25.0):
    rng = np.random.default_rng(0)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    for i in range(n):
        base = 0.5 + 0.35 * np.sin(x / (29 + i)) * np.cos(y / (41 + i)) + 0.1 * np.sin((x + y) / 11)
        img = np.stack([base, 1 - base, np.roll(base, 7 * i, 1)], -1) + rng.normal(0, sigma / 255.0, (h, w, 3))
        yield np.uint8(np.clip(img, 0, 1) * 255)


def make_folder(path, n, h, w):
    from PIL import Image
    for i, img in enumerate(make_pictures(n, h, w)):
        Image.fromarray(img).save(os.path.join(path, "img%04d.png" % i))


def depth_runs(a):
    """--depth both: the training loop fed from an 8-bit pool and from the 16-bit pool of the same pictures, alternating"""
    from ssdn.datasets import DevicePoolStream, ImagePool
    from ssdn.denoiser import Denoiser
    pictures = list(make_pictures(a.images, a.height, a.width))
    dev = torch.device("cuda", 0)
    pools = {8: ImagePool.from_images(pictures, dev), 16: ImagePool.from_images([p.astype(np.uint16) for p in pictures], dev, white=255)}
    cfg = ssdn.cfg.base()
    cfg[ConfigValue.ALGORITHM] = NoiseAlgorithm.SELFSUPERVISED_DENOISING
    cfg[ConfigValue.NOISE_STYLE] = "gauss25"
    cfg[ConfigValue.NOISE_VALUE] = NoiseValue.KNOWN
    torch.manual_seed(0)
    d = Denoiser(ssdn.cfg.infer(cfg, model_only=True), device="cuda:0")
    d.train()
    order = np.random.default_rng(1).integers(0, a.images, size=(a.steps + a.warmup, a.batch)).tolist()
    lines = []
    for r in range(a.rounds):
        for bits in (8, 16):
            stream = DevicePoolStream(pools[bits], order, NoiseAlgorithm.SELFSUPERVISED_DENOISING, "gauss25", a.patch, seed=5).attach(d)
            n, s = timed_loop(stream, a.warmup, lambda data: d.train_step(data, 3e-4, metrics=True))
            lines.append({"what": "train_pool", "bits": bits, "round": r, "images_per_s": round(n * a.batch / s, 1),
                          "ms_per_step": round(1e3 * s / n, 4), "minibatches": n, "pool_bytes": pools[bits].nbytes})
    med = {b: float(np.median([ln["images_per_s"] for ln in lines if ln["bits"] == b])) for b in (8, 16)}
    lines.append({"what": "medians", "images_per_s_8": med[8], "images_per_s_16": med[16], "ratio_16_over_8": round(med[16] / med[8], 4)})
    return lines


def make_trainer(folder, a, noisy, steps):
    from ssdn.train import DenoiserTrainer
    cfg = ssdn.cfg.base()
    cfg[ConfigValue.ALGORITHM] = NoiseAlgorithm.SELFSUPERVISED_DENOISING
    cfg[ConfigValue.NOISE_STYLE] = "gauss25"
    cfg[ConfigValue.NOISE_VALUE] = NoiseValue.KNOWN
    cfg[ConfigValue.TRAIN_DATA_PATH] = folder
    cfg[ConfigValue.TRAIN_ITERATIONS] = steps * a.batch
    cfg[ConfigValue.TRAIN_MINIBATCH_SIZE], cfg[ConfigValue.TRAIN_PATCH_SIZE] = a.batch, a.patch
    cfg[ConfigValue.DATALOADER_WORKERS] = a.workers
    torch.manual_seed(0)
    tr = DenoiserTrainer(cfg, runs_dir=os.path.join(folder, "_runs"))
    tr.noisy = noisy
    tr.new_target()
    tr.denoiser.train()
    return tr


def timed_loop(loader, warmup, body):
    """-> (minibatches timed, seconds): wall clock between two device synchronisations, the first `warmup` minibatches left out"""
    n, t0 = 0, None
    for data in loader:
        if n == warmup:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        body(data)
        n += 1
    torch.cuda.synchronize()
    return n - warmup, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=48)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=384)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--patch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=200, help="minibatches of (a) and (b) after the warm-up")
    ap.add_argument("--folder_steps", type=int, default=40, help="minibatches of (c) after the warm-up (every patch decodes a whole image)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workers", type=int, default=4, help="DataLoader workers of (c): the package's default")
    ap.add_argument("--depth", choices=["both"], help="8-bit pool against the 16-bit pool of the same pictures, alternating")
    ap.add_argument("--rounds", type=int, default=3, help="runs of each depth with --depth both")
    ap.add_argument("--out")
    a = ap.parse_args()
    from ssdn.hip import lib as L
    lines = [{"library_sha256": hashlib.sha256(open(L.LIB_PATH, "rb").read()).hexdigest(), "device": torch.cuda.get_device_name(0),
              "folder": "%d PNGs of %dx%d, gauss25 on a smooth picture" % (a.images, a.width, a.height), "batch": a.batch, "patch": a.patch}]
    lines += depth_runs(a) if a.depth else folder_runs(a)
    text = "\n".join(json.dumps(ln) for ln in lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


def folder_runs(a):
    lines = []
    with tempfile.TemporaryDirectory() as folder:
        make_folder(folder, a.images, a.height, a.width)
        # (a) and (b): the pool
        tr = make_trainer(folder, a, "style", a.steps + a.warmup)
        t0 = time.perf_counter()
        stream, _, _ = tr.train_data()
        build_s = time.perf_counter() - t0
        stream._denoiser = None                                   # (a): a buffer of its own per minibatch, nothing consumes it
        n, s = timed_loop(stream, a.warmup, lambda data: None)
        lines.append({"what": "pool_stream", "patches_per_s": round(n * a.batch / s, 1), "minibatches": n, "pool_bytes": stream.pool.nbytes,
                      "pool_build_s": round(build_s, 3)})
        tr = make_trainer(folder, a, "style", a.steps + a.warmup)
        stream, _, _ = tr.train_data()
        d = tr.denoiser
        n, s = timed_loop(stream, a.warmup, lambda data: d.train_step(data, 3e-4, metrics=True))
        lines.append({"what": "train_pool", "images_per_s": round(n * a.batch / s, 1), "ms_per_step": round(1e3 * s / n, 4), "minibatches": n})
        # (c): the folder through the DataLoader workers, noise synthesised on the device
        tr = make_trainer(folder, a, None, a.folder_steps + a.warmup)
        loader, _, _ = tr.train_data()
        d = tr.denoiser
        n, s = timed_loop(loader, a.warmup, lambda data: d.train_step(data, 3e-4, metrics=True))
        lines.append({"what": "train_folder", "images_per_s": round(n * a.batch / s, 1), "ms_per_step": round(1e3 * s / n, 4), "minibatches": n,
                      "workers": a.workers})
        del loader
    return lines


if __name__ == "__main__":
    main()
