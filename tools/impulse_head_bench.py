"""Time the impulse loss head (k_head_impulse<3>, k_head_vjp_impulse<false, 3>) next to the gauss one (k_head<false>,
k_head_vjp<false, false>) at BASELINE config-2 size (B = 32, 64x64, 3 channels, sigma / alpha known), on the same network output and noisy
image; the VJPs take all three upstream gradients (LOSS, posterior mean, mu).  Prints one JSON line of CUDA-event times per op list, the
algorithmic HBM bytes and the share of `--hbm-gbs` (default 8000: the MI355X's 8 TB/s) each launch achieves.
--trace DIR: runs itself once under `rocprofv3 --kernel-trace --stats` (a child process) and prints the kernel statistics of the four
head kernels from that one trace as a second JSON line (the trace files stay in DIR)."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "selfsupervised-denoising_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)


def run(args):
    import torch
    import restate as R
    from ssdn.hip import lib as L
    from ssdn.hip.engine import OpList, current_stream, HEAD_PX_PER_BLOCK
    B, P, C = args.batch, args.patch, 3
    HW = P * P
    dev = torch.device("cuda")
    f = dict(dtype=torch.float32, device=dev)
    mu = R.hash_tensor((B, C, P, P), 202, 0.05, 0.95)
    full = R.hash_tensor((B, 9, P, P), 201, -0.4, 0.6)
    full[:, :C] = mu
    full = full.to(dev)
    noisy = R.hash_tensor((B, C, P, P), 203, 0, 1).to(dev)
    npars = {"gauss": torch.full((B,), 25 / 255.0, **f), "impulse": torch.full((B,), 0.5, **f)}
    w = torch.randn(B, **f)
    gp, gm = torch.randn(B, C, P, P, **f), torch.randn(B, C, P, P, **f)
    nchunks = max(1, min(64, HW // HEAD_PX_PER_BLOCK))
    partial = torch.zeros(B, nchunks, 2, **f)
    gmax = torch.zeros(4, dtype=torch.int32, device=dev)
    mo, pme, mstd, nstd, loss = (torch.zeros(B, C, P, P, **f), torch.zeros(B, C, P, P, **f), torch.zeros(B, P, P, **f), torch.zeros(B, **f),
                                 torch.zeros(B, **f))
    p = lambda t: t.data_ptr()     # noqa: E731
    lists = {}
    g = torch.zeros(B, 9, P, P, **f)
    for name, sty in (("gauss", 0), ("impulse", 2)):
        npar = npars[name]
        lists["head_" + name] = OpList([("head_ssdn", L.HeadArgs(p(full), p(noisy), p(npar), None, B, C, P, P, sty, 0, 1, p(mo), p(pme), p(mstd),
                                                                 p(nstd), p(g), p(partial), nchunks, p(gmax), 0)),
                                        ("head_final", L.HeadFinalArgs(p(partial), B, nchunks, P, P, 0, p(loss), None, None, None))])
        a = L.HeadVjpArgs(p(full), p(noisy), p(npar), None, B, C, P, P, sty, 0, p(w), p(gp), p(gm), 0, nchunks, p(g), p(partial), p(gmax),
                          None, None, None)
        lists["vjp_" + name] = OpList([("head_vjp", a)])

    def timed(ol):
        s = current_stream()
        for _ in range(args.warmup):
            ol.run(s)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.iters):
            ol.run(s)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.iters
    res = dict(B=B, P=P, iters=args.iters)
    for k in ("head_gauss", "head_impulse", "vjp_gauss", "vjp_impulse"):
        res[k + "_us"] = round(timed(lists[k]), 2)
    # algorithmic HBM bytes, the same for both models: forward reads net_out + noisy (12 floats per pixel), writes mu, pme, model_std, g_net_out
    # (16); the VJP reads net_out, noisy, g_pme, g_mu (18) and writes g_net_out (9).  (the event times of the head lists include head_final)
    res["hbm_bytes_head"] = 4 * B * HW * (9 + C + C + C + 1 + 9)
    res["hbm_bytes_vjp"] = 4 * B * HW * (9 + C + C + C + 9)
    for k in ("head_gauss", "head_impulse", "vjp_gauss", "vjp_impulse"):
        res[k + "_hbm_share"] = round(res["hbm_bytes_" + k.split("_")[0]] / (res[k + "_us"] * 1e-6) / (args.hbm_gbs * 1e9), 4)
    print(json.dumps(res))


def trace(args):
    os.makedirs(args.trace, exist_ok=True)
    cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "-d", args.trace, "-o", "impulse_head", "--output-format", "csv",
           "--", sys.executable, os.path.abspath(__file__), "--batch", str(args.batch), "--patch", str(args.patch), "--iters", str(args.iters),
           "--warmup", str(args.warmup)]
    r = subprocess.run(cmd)
    if r.returncode != 0:
        sys.exit("rocprofv3 run failed with exit status %d" % r.returncode)
    stats = sorted(glob.glob(os.path.join(args.trace, "**", "*kernel_stats.csv"), recursive=True), key=os.path.getmtime)
    if not stats:
        sys.exit("no kernel_stats.csv under " + args.trace)
    out = {}
    with open(stats[-1]) as fh:
        for row in csv.DictReader(fh):
            name = row["Name"]
            if name.startswith(("k_head<false", "k_head_vjp<false, false", "void k_head<false", "void k_head_vjp<false, false", "k_head_impulse", "k_head_vjp_impulse",
                                "void k_head_impulse", "void k_head_vjp_impulse")):
                out[name] = dict(calls=int(row["Calls"]), avg_us=round(float(row["AverageNs"]) / 1e3, 2),
                                 min_us=round(float(row["MinNs"]) / 1e3, 2), max_us=round(float(row["MaxNs"]) / 1e3, 2))
    print(json.dumps(dict(kernel_stats=out, source=os.path.relpath(stats[-1], ROOT) if stats[-1].startswith(ROOT) else stats[-1])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--patch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="HBM bandwidth the achieved share is stated against, GB/s")
    ap.add_argument("--trace", metavar="DIR", default=None, help="run once under rocprofv3 --kernel-trace --stats and summarise")
    args = ap.parse_args()
    if args.trace:
        trace(args)
    else:
        run(args)


if __name__ == "__main__":
    main()
