"""Time NoiseNetwork's autograd backward at BASELINE config-2 size (B = 32, 64x64, blind-spot, 3 -> 9 channels) with and without the input
gradient (SSDN_OP_INPUT_GRAD), and the forward-only path for reference.  Prints one JSON line.  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/input_grad_bench.py` for the k_input_grad kernel time."""
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    import restate as R
    from ssdn.models.noise_network import NoiseNetwork
    B, P = args.batch, args.patch
    net = NoiseNetwork(3, 9, blindspot=True, device="cuda")
    net.load_state_dict(R.reference_state_dict(R.make_params(3, 9, True, seed=11)))
    x = R.hash_tensor((B, 3, P, P), 191, 0, 1).cuda()
    g = (R.hash_tensor((B, 9, P, P), 192, -1, 1) * 1e-3).cuda()

    def time_backward(xg):
        ts = []
        for i in range(args.warmup + args.iters):
            xd = x.clone().requires_grad_(xg)
            out = net(xd)
            net.zero_grad(set_to_none=True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            out.backward(g)
            e1.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                ts.append(e0.elapsed_time(e1))
        ts.sort()
        return ts[len(ts) // 2]

    res = dict(B=B, P=P, backward_ms_params_only=time_backward(False), backward_ms_with_input_grad=time_backward(True))
    res["input_grad_cost_ms"] = res["backward_ms_with_input_grad"] - res["backward_ms_params_only"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
