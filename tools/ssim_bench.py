"""Time the SSIM op (k_ssim + k_ssim_final, csrc/ssim.hip) at the evaluator's sizes, B = 4, C = 3 at 512 x 512 (BSD300)
and 768 x 768 (Kodak), without and with the SSIM map, next to k_metrics (SSDN_OP_METRICS: the PSNR pass, "one pass over the images") on
the same tensors in the same run.  Prints one JSON line of device-event times per op list, the algorithmic HBM bytes (two images in, the
map's centres out) and the share of `--hbm-gbs` (default 6300: the achievable HBM rate of the MI355X) each achieves.
--trace DIR: runs itself once under `rocprofv3 --kernel-trace --stats` (a child process, nothing else traced), splits the kernel trace by
kernel, image size and map / no map (the child's launch order is fixed: per size, every no-map launch before the first map launch) and
prints the per-kernel times as a second JSON line; --csv FILE also writes them as a table (the trace files stay in DIR)."""
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

SIZES = (512, 768)


def run(args):
    import torch
    import restate as R
    from ssdn.hip import lib as L
    from ssdn.hip.engine import OpList, current_stream
    B, C = args.batch, 3
    dev = torch.device("cuda")
    f = dict(dtype=torch.float32, device=dev)
    p = lambda t: t.data_ptr()     # noqa: E731
    res = dict(B=B, C=C, iters=args.iters)
    for S in SIZES:
        ref = R.hash_tensor((B, C, S, S), 301, 0, 1).to(dev)
        x = (ref + R.hash_tensor((B, C, S, S), 302, -1, 1).to(dev) * 0.1).contiguous()
        val, smap = torch.zeros(B, **f), torch.zeros(B, C, S, S, **f)
        nb = L.ssim_scratch_bytes(B, C, S, S)
        scratch = torch.zeros(nb // 8, dtype=torch.float64, device=dev)
        per, acc = torch.zeros(B, 8, **f), torch.zeros(16, **f)
        ssim = lambda m: L.SsimArgs(p(x), p(ref), None, B, C, S, S, p(val), p(smap) if m else None, p(scratch), nb)      # noqa: E731
        margs = L.MetricsArgs()
        margs.out, margs.clean, margs.B, margs.C, margs.H, margs.W, margs.per, margs.acc = p(x), p(ref), B, C, S, S, p(per), p(acc)
        lists = {"ssim": OpList([("ssim", ssim(False))]), "ssim_map": OpList([("ssim", ssim(True))]), "metrics": OpList([("metrics", margs)])}
        px = B * C * S * S
        nbytes = {"ssim": 8 * px, "ssim_map": 8 * px + 4 * B * C * (S - 10) * (S - 10), "metrics": 8 * px}
        for k, ol in lists.items():          # (this order: the trace is split by it)
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
            us = e0.elapsed_time(e1) * 1e3 / args.iters
            key = "%s_%d" % (k, S)
            res[key + "_us"] = round(us, 2)
            res[key + "_hbm_bytes"] = nbytes[k]
            res[key + "_hbm_share"] = round(nbytes[k] / (us * 1e-6) / (args.hbm_gbs * 1e9), 4)
        res["ssim_%d_fp64_flop" % S] = 2 * 220 * B * C * (S - 10) * (S - 10)
    print(json.dumps(res))


def trace(args):
    os.makedirs(args.trace, exist_ok=True)
    cmd = ["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "-d", args.trace, "-o", "ssim", "--output-format", "csv",
           "--", sys.executable, os.path.abspath(__file__), "--batch", str(args.batch), "--iters", str(args.iters), "--warmup", str(args.warmup)]
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
            if name.startswith(("k_ssim", "k_metrics")):
                rows.append((int(row["Start_Timestamp"]), name.split("(")[0], int(row["End_Timestamp"]) - int(row["Start_Timestamp"]),
                             row.get("VGPR_Count"), row.get("LDS_Block_Size")))
    rows.sort()
    per = args.warmup + args.iters
    out, table = {}, []
    for name in ("k_ssim", "k_ssim_final", "k_metrics"):
        mine = [r for r in rows if r[1] == name]
        configs = [(S, m) for S in SIZES for m in (("nomap", "map") if name != "k_metrics" else ("",))]
        if len(mine) != per * len(configs):
            sys.exit("%s: %d dispatches in the trace, expected %d" % (name, len(mine), per * len(configs)))
        for i, (S, m) in enumerate(configs):
            d = [r[2] for r in mine[i * per + args.warmup:(i + 1) * per]]
            key = "%s_%d%s" % (name, S, "_" + m if m else "")
            out[key] = dict(calls=len(d), avg_us=round(sum(d) / len(d) / 1e3, 2), min_us=round(min(d) / 1e3, 2), max_us=round(max(d) / 1e3, 2),
                            vgprs=mine[0][3], lds_bytes=mine[0][4])
            table.append([name, S, m or "-", len(d), "%.1f" % (sum(d) / len(d)), min(d), max(d), mine[0][3], mine[0][4]])
    if args.csv:
        with open(args.csv, "w", newline="") as fh:
            w = csv.writer(fh)
            w.writerow(["Kernel", "Size", "Map", "Calls", "AverageNs", "MinNs", "MaxNs", "VGPR_Count", "LDS_Block_Size"])
            w.writerows(table)
    print(json.dumps(dict(kernel_times=out, source=os.path.basename(traces[-1]))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--hbm-gbs", type=float, default=6300.0, help="HBM bandwidth the achieved share is stated against, GB/s")
    ap.add_argument("--trace", metavar="DIR", default=None, help="run once under rocprofv3 --kernel-trace --stats and summarise")
    ap.add_argument("--csv", metavar="FILE", default=None, help="with --trace: also write the per-kernel table there")
    args = ap.parse_args()
    if args.trace:
        trace(args)
    else:
        run(args)


if __name__ == "__main__":
    main()
