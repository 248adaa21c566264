"""Time whole-image denoising for an ssdn gauss25 known-sigma RGB model with random weights over `--images` noisy
images of 512 x 512 and of 768 x 768, one image per batch: per image, between device events (which also cover the host work in between),
  host    -- the host route the tests compare against: to_tensor, permute, pad_to_output_size, fp32 upload, run_pipeline, fp32
             download, unpad, tensor2image;
  denoise -- Denoiser.denoise: packed bytes up, SSDN_OP_IMAGE_IN, the same plan, SSDN_OP_IMAGE_OUT, bytes down;
  network -- the plan's forward list alone on the input already in place: the floor.
--auto adds the estimator's leg: after those three, Denoiser.denoise with the number and with noise_param="auto"
(SSDN_OP_NOISE_EST between SSDN_OP_IMAGE_IN and the run) alternate twice; `denoise_alt_*` and `auto_*` are the lists of both.
Prints one JSON line.  --trace DIR: runs itself once under `rocprofv3 --kernel-trace --stats` (a child process, nothing else traced) and
prints the times of k_image_in / k_image_out per size with their algorithmic HBM bytes (in: 1 byte read and 4 written per padded element;
out: 4 read and 1 written per element of the extent; with --auto also k_noise_est: 1 byte read per element, and k_noise_est_final: the
32 KiB table) and the share of `--hbm-gbs` they achieve; --csv FILE also writes that table.
--tile measures tiled denoising instead, same model: cost -- a 1024 x 768 image untiled and with tile = 256 and 512
at the default overlap, at batch sizes 1 and 4, ms per image between device events next to the tile count and the compute overhead
Kx Ky T^2 / (w h) the overlap implies; big -- one 4096 x 3072 image, tiled only (tile 512), with its time and the peak device memory;
fidelity -- a 768 x 768 noisy synthetic picture, tile 256 with overlap 0, 32, 64 and 128 against the untiled output: PSNR in dB over the
bytes and the largest byte difference (random weights: how fast a tile border's influence decays, nothing about a trained model).  With
--trace DIR it runs itself once under rocprofv3 and prints the times of k_tile_in / k_tile_out per kernel and grid."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "selfsupervised-denoising_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

SIZES = (512, 768)


def run(args):
    import numpy as np
    import torch
    from PIL import Image
    import ssdn
    from ssdn.datasets import NoisyDataset
    from ssdn.datasets.transforms import to_tensor
    from ssdn.denoiser import Denoiser
    from ssdn.params import ConfigValue, NoiseAlgorithm, NoiseValue, PipelineOutput
    from ssdn.utils import tensor2image
    cfg = ssdn.cfg.base()
    cfg[ConfigValue.ALGORITHM] = NoiseAlgorithm.SELFSUPERVISED_DENOISING
    cfg[ConfigValue.NOISE_STYLE] = "gauss25"
    cfg[ConfigValue.NOISE_VALUE] = NoiseValue.KNOWN
    torch.manual_seed(0)
    d = Denoiser(ssdn.cfg.infer(cfg, model_only=True), device="cuda:0")
    d.eval()
    g = np.random.default_rng(0)
    res = dict(images=args.images)
    MD = NoisyDataset.Metadata
    meta = {MD.INPUT_NOISE_VALUES: torch.full((1, 1, 1, 1), 25 / 255)}
    nd = NoisyDataset(None, "gauss25", None, pad_multiple=32, square=True)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.images, (time.perf_counter() - t0) * 1e3 / args.images

    for S in SIZES:
        images = [g.integers(0, 256, size=(S, S, 3), dtype=np.uint8) for _ in range(args.images)]

        def host():
            out = []
            for im in images:
                x = nd.pad_to_output_size(to_tensor(Image.fromarray(im)).permute(0, 2, 1))
                shape = torch.tensor([list(x.shape)])
                with torch.no_grad():
                    o = d.run_pipeline([x[None].to(d.device), torch.zeros(0), meta])[PipelineOutput.IMG_DENOISED].cpu()
                out.append(np.asarray(tensor2image(NoisyDataset.unpad(o, {MD.IMAGE_SHAPE: shape}, 0))))
            return out

        def device():
            return d.denoise(images, noise_param=25)["out"]

        a, b = host(), device()                                   # warm-up: the plan, the pinned buffers
        assert all(np.array_equal(x, y.numpy()) for x, y in zip(a, b)), "the two routes differ"
        eng = d._engines[(1, S, S, False, 64)][0]

        def network():
            for _ in range(args.images):
                eng.forward()
        network()
        for name, fn in (("host", host), ("denoise", device), ("network", network)):
            ev, wall = timed(fn)
            res["%s_%d_ms" % (name, S)] = round(ev, 3)
            res["%s_%d_wall_ms" % (name, S)] = round(wall, 3)
        if args.auto:
            def auto():
                return d.denoise(images, noise_param="auto")

            used = auto()["noise_param"]                             # warm-up: the estimator's buffers
            res["auto_param_%d" % S] = [round(min(used) * 255, 3), round(max(used) * 255, 3)]
            for _ in range(2):
                for name, fn in (("denoise_alt", device), ("auto", auto)):
                    ev, wall = timed(fn)
                    res.setdefault("%s_%d_ms" % (name, S), []).append(round(ev, 3))
                    res.setdefault("%s_%d_wall_ms" % (name, S), []).append(round(wall, 3))
    print(json.dumps(res))


def run_tile(args):
    import numpy as np
    import torch
    import ssdn
    from ssdn.denoiser import Denoiser
    from ssdn.hip import lib as L
    from ssdn.params import ConfigValue, NoiseAlgorithm, NoiseValue
    cfg = ssdn.cfg.base()
    cfg[ConfigValue.ALGORITHM] = NoiseAlgorithm.SELFSUPERVISED_DENOISING
    cfg[ConfigValue.NOISE_STYLE] = "gauss25"
    cfg[ConfigValue.NOISE_VALUE] = NoiseValue.KNOWN
    torch.manual_seed(0)
    d = Denoiser(ssdn.cfg.infer(cfg, model_only=True), device="cuda:0")
    d.eval()
    g = np.random.default_rng(0)
    res = dict(images=args.images)

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return round(e0.elapsed_time(e1) / n, 3)

    def picture(h, w):
        """something smooth with edges plus gaussian noise of sigma 25, as bytes"""
        yy, xx = np.mgrid[0:h, 0:w]
        clean = 128 + 70 * np.sin(xx / 37.0) * np.cos(yy / 23.0) + 40 * ((xx // 96 + yy // 64) % 2)
        return np.clip(clean[:, :, None] + g.normal(0, 25, (h, w, 3)), 0, 255).astype(np.uint8)

    # cost
    w, h = 1024, 768
    img = [picture(h, w)]
    d.denoise(img, noise_param=25)
    res["untiled_1024x768_ms"] = timed(lambda: d.denoise(img, noise_param=25), args.images)
    for T in (256, 512):
        O = Denoiser._tile_options(T, None)[1]
        n = L.tile_count(w, T, O) * L.tile_count(h, T, O)
        for bs in (1, 4):
            fn = lambda: d.denoise(img, noise_param=25, tile=T, batch_size=bs)      # noqa: E731
            fn()
            res["tile%d_o%d_b%d_1024x768" % (T, O, bs)] = dict(ms=timed(fn, args.images), tiles=n, overhead=round(n * T * T / (w * h), 3))
    d._engines.clear()
    # fidelity
    pic = [picture(768, 768)]
    ref = d.denoise(pic, noise_param=25)["out"][0].numpy().astype(np.float64)
    for O in (0, 32, 64, 128):
        out = d.denoise(pic, noise_param=25, tile=256, overlap=O, batch_size=4)["out"][0].numpy().astype(np.float64)
        mse = float(((out - ref) ** 2).mean())
        res["fidelity_768_t256_o%d" % O] = dict(psnr_db=round(10 * np.log10(255.0 ** 2 / mse), 2) if mse > 0 else None,
                                                max_byte_diff=int(np.abs(out - ref).max()), differing=round(float((out != ref).mean()), 4))
    d._engines.clear()
    torch.cuda.empty_cache()
    # big: beyond the untiled route's tested range, tiled only
    w, h, T = 4096, 3072, 512
    O = Denoiser._tile_options(T, None)[1]
    big = [picture(h, w)]
    torch.cuda.reset_peak_memory_stats()
    fn = lambda: d.denoise(big, noise_param=25, tile=T, batch_size=4)      # noqa: E731
    fn()
    res["tile%d_o%d_b4_4096x3072" % (T, O)] = dict(ms=timed(fn, 3), tiles=L.tile_count(w, T, O) * L.tile_count(h, T, O),
                                                  peak_device_MB=round(torch.cuda.max_memory_allocated() / 2 ** 20, 1))
    print(json.dumps(res))


def trace_tile(args):
    os.makedirs(args.trace, exist_ok=True)
    cmd = ["timeout", "-k", "10", "400", "rocprofv3", "--kernel-trace", "--stats", "-d", args.trace, "-o", "tile", "--output-format", "csv",
           "--", sys.executable, os.path.abspath(__file__), "--tile", "--images", str(args.images)]
    r = subprocess.run(cmd)
    if r.returncode != 0:
        sys.exit("rocprofv3 run failed with exit status %d" % r.returncode)
    traces = sorted(glob.glob(os.path.join(args.trace, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    if not traces:
        sys.exit("no kernel_trace.csv under " + args.trace)
    groups = {}
    with open(traces[-1]) as fh:
        for row in csv.DictReader(fh):
            name = row["Kernel_Name"]
            name = name[5:] if name.startswith("void ") else name
            if name.startswith("k_tile_"):
                grid = "x".join(str(row.get(k, "?")) for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z"))
                groups.setdefault((name.split("(")[0], grid), []).append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    out = {}
    for (name, grid), dur in sorted(groups.items()):
        dur = dur[1:] if len(dur) > 1 else dur                     # (the first launch of a kind loads the code object / a cold cache)
        out["%s grid %s" % (name, grid)] = dict(calls=len(dur), avg_us=round(sum(dur) / len(dur) / 1e3, 2), min_us=round(min(dur) / 1e3, 2),
                                               max_us=round(max(dur) / 1e3, 2))
    print(json.dumps(dict(kernel_times=out, source=os.path.basename(traces[-1]))))


def trace(args):
    os.makedirs(args.trace, exist_ok=True)
    cmd = ["timeout", "-k", "10", "400", "rocprofv3", "--kernel-trace", "--stats", "-d", args.trace, "-o", "denoise", "--output-format", "csv",
           "--", sys.executable, os.path.abspath(__file__), "--images", str(args.images)] + (["--auto"] if args.auto else [])
    r = subprocess.run(cmd)
    if r.returncode != 0:
        sys.exit("rocprofv3 run failed with exit status %d" % r.returncode)
    traces = sorted(glob.glob(os.path.join(args.trace, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    if not traces:
        sys.exit("no kernel_trace.csv under " + args.trace)
    rows = []
    with open(traces[-1]) as fh:
        for row in csv.DictReader(fh):
            name = row["Kernel_Name"]
            name = name[5:] if name.startswith("void ") else name
            if name.startswith("k_image_") or name.startswith("k_noise_est"):
                rows.append((int(row["Start_Timestamp"]), name.split("<")[0].split("(")[0], int(row["End_Timestamp"]) - int(row["Start_Timestamp"]),
                             row.get("VGPR_Count"), row.get("LDS_Block_Size")))
    rows.sort()
    # passes of Denoiser.denoise per size: the warm-up and the timed one; with --auto the estimator's warm-up and two alternations more
    passes = {"k_image_in": 7 if args.auto else 2, "k_image_out": 7 if args.auto else 2}
    if args.auto:
        passes.update(k_noise_est=3, k_noise_est_final=3)
    out, table = {}, []
    for name, n in passes.items():
        per = n * args.images
        mine = [r for r in rows if r[1] == name]
        if len(mine) != per * len(SIZES):
            sys.exit("%s: %d dispatches in the trace, expected %d" % (name, len(mine), per * len(SIZES)))
        for i, S in enumerate(SIZES):
            dur = [r[2] for r in mine[i * per + 1:(i + 1) * per]]         # (the first launch of a size loads the code object / a cold cache)
            nbytes = {"k_noise_est": 3 * S * S, "k_noise_est_final": 8 * 1024 * 4 + 8 * 8 + 20 * 8 + 4}.get(name, 5 * 3 * S * S)
            avg = sum(dur) / len(dur)
            out["%s_%d" % (name, S)] = dict(calls=len(dur), avg_us=round(avg / 1e3, 2), min_us=round(min(dur) / 1e3, 2),
                                            max_us=round(max(dur) / 1e3, 2), hbm_bytes=nbytes, gbs=round(nbytes / avg, 1),
                                            hbm_share=round(nbytes / avg / args.hbm_gbs, 4), vgprs=mine[0][3], lds_bytes=mine[0][4])
            table.append([name, S, len(dur), "%.1f" % avg, min(dur), max(dur), nbytes, "%.1f" % (nbytes / avg), mine[0][3], mine[0][4]])
    if args.csv:
        with open(args.csv, "w", newline="") as fh:
            w = csv.writer(fh)
            w.writerow(["Kernel", "Size", "Calls", "AverageNs", "MinNs", "MaxNs", "HbmBytes", "GBperS", "VGPR_Count", "LDS_Block_Size"])
            w.writerows(table)
    print(json.dumps(dict(kernel_times=out, source=os.path.basename(traces[-1]))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=20)
    ap.add_argument("--hbm-gbs", type=float, default=6300.0, help="HBM bandwidth the achieved share is stated against, GB/s")
    ap.add_argument("--auto", action="store_true", help="also time Denoiser.denoise(noise_param='auto'), alternating with the number")
    ap.add_argument("--trace", metavar="DIR", default=None, help="run once under rocprofv3 --kernel-trace --stats and summarise")
    ap.add_argument("--csv", metavar="FILE", default=None, help="with --trace: also write the per-kernel table there")
    ap.add_argument("--tile", action="store_true", help="measure tiled denoising instead: cost, one large image, fidelity against the untiled output")
    args = ap.parse_args()
    if args.tile:
        (trace_tile if args.trace else run_tile)(args)
    elif args.trace:
        trace(args)
    else:
        run(args)


if __name__ == "__main__":
    main()
