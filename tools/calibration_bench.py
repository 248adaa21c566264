"""Time the calibration op (k_calib + k_calib_final, csrc/calibration.hip) at the evaluator's Kodak size, B = 1, C = 3,
768 x 768, without and with the histogram and the z-map, next to SSDN_OP_SSIM on tensors of the same size in the same run -- the method of
tools/ssim_bench.py: device events around `--iters` back-to-back op lists after `--warmup`.  Prints one JSON line: microseconds per op
list, the algorithmic HBM bytes (mean, cov and ref in: 48 bytes per RGB pixel; the z-map out) and the share of `--hbm-gbs` each achieves."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "selfsupervised-denoising_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--size", type=int, default=768)
    ap.add_argument("--iters", type=int, default=2000)           # (a launch-bound op: a window of tens of milliseconds)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--hbm-gbs", type=float, default=6300.0, help="HBM bandwidth the achieved share is stated against, GB/s")
    args = ap.parse_args()
    import torch
    import restate as R
    from ssdn.hip import lib as L
    from ssdn.hip.engine import OpList, current_stream
    B, C, S = args.batch, 3, args.size
    dev = torch.device("cuda")
    p = lambda t: t.data_ptr()     # noqa: E731
    ref = R.hash_tensor((B, C, S, S), 301, 0, 1).to(dev)
    mean = (ref + R.hash_tensor((B, C, S, S), 302, -1, 1).to(dev) * 0.1).contiguous()
    cov = torch.zeros(B, 6, S, S, device=dev)
    cov[:, [0, 3, 5]] = 0.01 + 0.01 * R.hash_tensor((B, 3, S, S), 303, 0, 1).to(dev)           # a well-conditioned covariance: sd ~ the residual
    cov[:, [1, 2, 4]] = 0.003 * R.hash_tensor((B, 3, S, S), 304, -1, 1).to(dev)
    stats = torch.zeros(B, L.CALIB_NSTATS, dtype=torch.float64, device=dev)
    hist = torch.zeros(B, C, L.CALIB_HIST_BINS, dtype=torch.int64, device=dev)
    zmap = torch.zeros(B, C, S, S, device=dev)
    nb = L.calib_scratch_bytes(B, C, S, S)
    scratch = torch.zeros(nb // 8, dtype=torch.float64, device=dev)
    val, smap = torch.zeros(B, device=dev), torch.zeros(B, C, S, S, device=dev)
    nbs = L.ssim_scratch_bytes(B, C, S, S)
    sscratch = torch.zeros(nbs // 8, dtype=torch.float64, device=dev)
    calib = lambda h, m: L.CalibrationArgs(p(mean), p(cov), p(ref), None, B, C, S, S, p(stats), p(hist) if h else None,      # noqa: E731
                                           p(zmap) if m else None, p(scratch), nb)
    lists = {"calibration": OpList([("calibration", calib(False, False))]), "calibration_hist_map": OpList([("calibration", calib(True, True))]),
             "ssim": OpList([("ssim", L.SsimArgs(p(mean), p(ref), None, B, C, S, S, p(val), None, p(sscratch), nbs))])}
    px = B * S * S
    nbytes = {"calibration": 48 * px, "calibration_hist_map": 60 * px, "ssim": 8 * C * px}
    res = dict(B=B, C=C, size=S, iters=args.iters, device=torch.cuda.get_device_name(0))
    for k, ol in lists.items():
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
        res[k + "_us"] = round(us, 2)
        res[k + "_hbm_bytes"] = nbytes[k]
        res[k + "_hbm_share"] = round(nbytes[k] / (us * 1e-6) / (args.hbm_gbs * 1e9), 4)
    res["maha"] = round(float(stats[0, 2] / (stats[0, 0] * C)), 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
