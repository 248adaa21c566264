"""Time the posterior op (k_head_posterior<1, false> without samples, k_head_posterior<1, true> with S = 8) next to
the forward loss head k_head<false> at BASELINE config-2 size (B = 32, 64x64, 3 channels, gauss, sigma known), on the same network output
and noisy image.  Prints one JSON line of CUDA-event times per op list, the algorithmic HBM bytes (12 floats in, 9 out, + 3 S for samples,
per pixel) and the share of `--hbm-gbs` (default 6300: the achievable HBM rate of the MI355X) each launch achieves.
--trace DIR: runs itself once under `rocprofv3 --kernel-trace --stats` (a child process, nothing else traced) and prints the kernel
statistics of the three kernels from that one trace as a second JSON line (the trace files stay in DIR)."""
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
    B, P, C, S = args.batch, args.patch, 3, args.samples
    HW = P * P
    dev = torch.device("cuda")
    f = dict(dtype=torch.float32, device=dev)
    full = R.hash_tensor((B, 9, P, P), 201, -0.4, 0.6)
    full[:, :C] = R.hash_tensor((B, C, P, P), 202, 0.05, 0.95)
    full = full.to(dev)
    noisy = R.hash_tensor((B, C, P, P), 203, 0, 1).to(dev)
    npar = torch.full((B,), 25 / 255.0, **f)
    nchunks = max(1, min(64, HW // HEAD_PX_PER_BLOCK))
    partial = torch.zeros(B, nchunks, 2, **f)
    gmax = torch.zeros(4, dtype=torch.int32, device=dev)
    mo, pme, mstd, nstd = torch.zeros(B, C, P, P, **f), torch.zeros(B, C, P, P, **f), torch.zeros(B, P, P, **f), torch.zeros(B, **f)
    cov, std, smp = torch.zeros(B, 6, P, P, **f), torch.zeros(B, C, P, P, **f), torch.zeros(S, B, C, P, P, **f)
    p = lambda t: t.data_ptr()     # noqa: E731
    post = lambda n: L.HeadPosteriorArgs(p(full), p(noisy), p(npar), None, B, C, P, P, 0, 0, 0, nchunks, p(cov), p(std),      # noqa: E731
                                         p(smp) if n else None, n, 1, 0)
    lists = {
        # the inference form of the loss head: no gradient (Denoiser.posterior's forward)
        "head": OpList([("head_ssdn", L.HeadArgs(p(full), p(noisy), p(npar), None, B, C, P, P, 0, 0, 0, p(mo), p(pme), p(mstd), p(nstd), None,
                                                 p(partial), nchunks, p(gmax), 0))]),
        "posterior": OpList([("head_posterior", post(0))]),
        "posterior_s%d" % S: OpList([("head_posterior", post(S))]),
    }

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
    res = dict(B=B, P=P, S=S, iters=args.iters)
    nbytes = {"head": 4 * B * HW * (12 + C + C + 1), "posterior": 4 * B * HW * (12 + 9), "posterior_s%d" % S: 4 * B * HW * (12 + 9 + 3 * S)}
    for k, ol in lists.items():
        res[k + "_us"] = round(timed(ol), 2)
        res[k + "_hbm_bytes"] = nbytes[k]
        res[k + "_hbm_share"] = round(nbytes[k] / (res[k + "_us"] * 1e-6) / (args.hbm_gbs * 1e9), 4)
    print(json.dumps(res))


def trace(args):
    os.makedirs(args.trace, exist_ok=True)
    cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "-d", args.trace, "-o", "posterior", "--output-format", "csv",
           "--", sys.executable, os.path.abspath(__file__), "--batch", str(args.batch), "--patch", str(args.patch), "--iters", str(args.iters),
           "--warmup", str(args.warmup), "--samples", str(args.samples)]
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
            if name.startswith(("k_head<false", "void k_head<false", "k_head_posterior", "void k_head_posterior")):
                out[name] = dict(calls=int(row["Calls"]), avg_us=round(float(row["AverageNs"]) / 1e3, 2),
                                 min_us=round(float(row["MinNs"]) / 1e3, 2), max_us=round(float(row["MaxNs"]) / 1e3, 2))
    print(json.dumps(dict(kernel_stats=out, source=os.path.relpath(stats[-1], ROOT) if stats[-1].startswith(ROOT) else stats[-1])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--patch", type=int, default=64)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--hbm-gbs", type=float, default=6300.0, help="HBM bandwidth the achieved share is stated against, GB/s")
    ap.add_argument("--trace", metavar="DIR", default=None, help="run once under rocprofv3 --kernel-trace --stats and summarise")
    args = ap.parse_args()
    if args.trace:
        trace(args)
    else:
        run(args)


if __name__ == "__main__":
    main()
