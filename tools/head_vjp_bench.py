"""Time the loss head's vector-Jacobian product (SSDN_OP_HEAD_VJP) at BASELINE config-2 size (B = 32, 64x64, 3 channels, gauss25, sigma
known) with all three upstream gradients (LOSS, posterior mean, mu), next to the forward's head (SSDN_OP_HEAD_SSDN) on the same data.
Prints one JSON line.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/head_vjp_bench.py` for the k_head_vjp kernel time."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "selfsupervised-denoising_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--patch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    import restate as R
    from ssdn.hip import lib as L
    from ssdn.hip.engine import OpList, current_stream, HEAD_PX_PER_BLOCK
    B, P, C = args.batch, args.patch, 3
    HW = P * P
    dev = torch.device("cuda")
    f = dict(dtype=torch.float32, device=dev)
    net_out = R.hash_tensor((B, 9, P, P), 201, -0.4, 0.6)
    net_out[:, :C] = R.hash_tensor((B, C, P, P), 202, 0.05, 0.95)
    net_out = net_out.to(dev)
    noisy = R.hash_tensor((B, C, P, P), 203, 0, 1).to(dev)
    npar = torch.full((B,), 25 / 255.0, **f)
    w = torch.randn(B, **f)
    gp, gm = torch.randn(B, C, P, P, **f), torch.randn(B, C, P, P, **f)
    nchunks = max(1, min(64, HW // HEAD_PX_PER_BLOCK))
    g = torch.zeros(B, 9, P, P, **f)
    partial = torch.zeros(B, nchunks, 2, **f)
    gmax = torch.zeros(4, dtype=torch.int32, device=dev)
    mu, pme, mstd, nstd, loss = (torch.zeros(B, C, P, P, **f), torch.zeros(B, C, P, P, **f), torch.zeros(B, P, P, **f), torch.zeros(B, **f),
                                 torch.zeros(B, **f))
    p = lambda t: t.data_ptr()     # noqa: E731
    vjp = OpList([("head_vjp", L.HeadVjpArgs(p(net_out), p(noisy), p(npar), None, B, C, P, P, 0, 0, p(w), p(gp), p(gm), 0, nchunks, p(g),
                                             p(partial), p(gmax), None, None, None))])
    head = OpList([("head_ssdn", L.HeadArgs(p(net_out), p(noisy), p(npar), None, B, C, P, P, 0, 0, 1, p(mu), p(pme), p(mstd), p(nstd), p(g),
                                            p(partial), nchunks, p(gmax))),
                   ("head_final", L.HeadFinalArgs(p(partial), B, nchunks, P, P, 0, p(loss), None, None, None))])

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
    res = dict(B=B, P=P, head_vjp_us=timed(vjp), head_fwd_us=timed(head))
    res["hbm_bytes_vjp"] = 4 * B * HW * (9 + C + C + C + 9)      # net_out, noisy, g_pme, g_mu in; g_net_out out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
