"""Time the risk op (k_risk + k_risk_final, csrc/risk.hip) at the evaluator's Kodak size, B = 1, C = 3, 768 x 768, for
the full and the diagonal covariance and both noise styles, next to SSDN_OP_CALIBRATION without histogram and map on tensors of the same size
in the same run -- the method of tools/calibration_bench.py: device events around `--iters` back-to-back op lists after `--warmup`.  Prints
one JSON line: microseconds per op list, the algorithmic HBM bytes (net_out, noisy and pme in: 60 bytes per RGB pixel with the full
covariance, 48 with the diagonal one; calibration: 48) and the share of `--hbm-gbs` each achieves."""
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
    ap.add_argument("--margin", type=int, default=16)
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
    ref = R.hash_tensor((B, C, S, S), 301, 0.05, 0.95).to(dev)
    noisy = (ref + R.hash_tensor((B, C, S, S), 302, -1, 1).to(dev) * 0.17).contiguous()
    net_out = torch.zeros(B, 9, S, S, device=dev)
    net_out[:, :3] = ref + R.hash_tensor((B, C, S, S), 305, -1, 1).to(dev) * 0.05
    net_out[:, [3, 6, 8]] = 0.03 + 0.03 * R.hash_tensor((B, 3, S, S), 303, 0, 1).to(dev)        # U: a well-conditioned Sigma_x
    net_out[:, [4, 5, 7]] = 0.02 * R.hash_tensor((B, 3, S, S), 304, -1, 1).to(dev)
    net_diag = net_out[:, :6].contiguous()
    pme = (0.6 * net_out[:, :3] + 0.4 * noisy).contiguous()
    npar = {0: torch.full((B,), 25 / 255.0, device=dev), 1: torch.full((B,), 30.0, device=dev)}
    stats = torch.zeros(B, L.RISK_NSTATS, dtype=torch.float64, device=dev)
    nb = L.risk_scratch_bytes(B, C, S, S)
    scratch = torch.zeros(nb // 8, dtype=torch.float64, device=dev)
    cov = torch.zeros(B, 6, S, S, device=dev)
    cov[:, [0, 3, 5]] = 0.01 + 0.01 * R.hash_tensor((B, 3, S, S), 303, 0, 1).to(dev)
    cov[:, [1, 2, 4]] = 0.003 * R.hash_tensor((B, 3, S, S), 304, -1, 1).to(dev)
    cstats = torch.zeros(B, L.CALIB_NSTATS, dtype=torch.float64, device=dev)
    cnb = L.calib_scratch_bytes(B, C, S, S)
    cscratch = torch.zeros(cnb // 8, dtype=torch.float64, device=dev)
    risk = lambda no, style, diag, margin: L.RiskArgs(p(no), p(noisy), p(npar[style]), None, p(pme), None, B, C, S, S, style, 0, diag,      # noqa: E731
                                                      margin, p(stats), p(scratch), nb)
    lists = {"risk_gauss_full": OpList([("risk", risk(net_out, 0, 0, args.margin))]),
             "risk_gauss_full_margin0": OpList([("risk", risk(net_out, 0, 0, 0))]),
             "risk_poisson_full": OpList([("risk", risk(net_out, 1, 0, args.margin))]),
             "risk_gauss_diag": OpList([("risk", risk(net_diag, 0, 1, args.margin))]),
             "calibration": OpList([("calibration", L.CalibrationArgs(p(pme), p(cov), p(ref), None, B, C, S, S, p(cstats), None, None,
                                                                      p(cscratch), cnb))])}
    px, pxm = B * S * S, B * (S - 2 * args.margin) ** 2
    nbytes = {"risk_gauss_full": 60 * pxm, "risk_gauss_full_margin0": 60 * px, "risk_poisson_full": 60 * pxm, "risk_gauss_diag": 48 * pxm,
              "calibration": 48 * px}
    res = dict(B=B, C=C, size=S, margin=args.margin, iters=args.iters, device=torch.cuda.get_device_name(0))
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
    vals = __import__("ssdn.utils", fromlist=["risk_values"]).risk_values(stats.cpu(), C)
    res["psnr_out_est"] = round(float(vals["psnr_out_est"][0]), 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
