"""Time the autograd backward of Denoiser.run_pipeline with and without an input gradient (x.requires_grad) at BASELINE config-2 size
(B = 32, 64x64, 3 channels, ssdn gauss25, sigma known) and config 3 (sigma variable: the sigma-estimation network too), all three upstream
gradients (LOSS, posterior mean, mu).  Prints one JSON line.  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/denoiser_input_grad_bench.py` for the k_head_vjp / k_input_grad kernel times."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "selfsupervised-denoising_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)


def make(mode, B, P):
    import torch
    import restate as R
    import ssdn
    from ssdn.denoiser import Denoiser
    from ssdn.datasets import NoisyDataset
    from ssdn.params import ConfigValue, NoiseAlgorithm, NoiseValue
    cfg = ssdn.cfg.base()
    cfg[ConfigValue.ALGORITHM] = NoiseAlgorithm.SELFSUPERVISED_DENOISING
    cfg[ConfigValue.NOISE_STYLE] = "gauss25"
    cfg[ConfigValue.NOISE_VALUE] = NoiseValue(mode)
    ssdn.cfg.infer(cfg, model_only=True)
    d = Denoiser(cfg, device="cuda:0")
    d.get_model(Denoiser.MODEL, False).load_state_dict(R.reference_state_dict(R.make_params(3, 9, True, seed=5)))
    if mode == "var":
        d.get_model(Denoiser.SIGMA_ESTIMATOR, False).load_state_dict(R.reference_state_dict(R.make_params(3, 1, False, seed=6)))
    d.mark_dirty()
    d.train()
    clean = R.hash_tensor((B, 3, P, P), 161, 0, 1)
    noisy = torch.clamp(clean + R.hash_tensor((B, 3, P, P), 162, -1, 1) * 0.17, 0, 1)
    meta = {NoisyDataset.Metadata.CLEAN: clean, NoisyDataset.Metadata.INPUT_NOISE_VALUES: torch.full((B, 1, 1, 1), 25 / 255.0)}
    return d, [noisy.cuda(), clean.cuda(), meta]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--patch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--modes", default="known,var")
    args = ap.parse_args()
    import torch
    from ssdn.params import PipelineOutput as PO
    B, P = args.batch, args.patch
    g = torch.Generator(device="cuda").manual_seed(0)
    w = torch.randn(B, device="cuda", generator=g)
    gp = 1e-2 * torch.randn(B, 3, P, P, device="cuda", generator=g)
    gm = 1e-2 * torch.randn(B, 3, P, P, device="cuda", generator=g)
    res = dict(B=B, P=P)
    for mode in args.modes.split(","):
        d, data = make(mode, B, P)
        for xg in (False, True):
            x = data[0].detach().clone().requires_grad_(xg)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t = 0.0
            for i in range(args.warmup + args.iters):
                out = d.run_pipeline([x] + data[1:])
                L = (out[PO.LOSS].view(B) * w).sum() + (out[PO.IMG_DENOISED] * gp).sum() + (out[PO.IMG_MU] * gm).sum()
                torch.cuda.synchronize()
                e0.record()
                L.backward()          # the backward node: VJP + backward lists (+ the input-gradient ops, x.grad)
                e1.record()
                torch.cuda.synchronize()
                if i >= args.warmup:
                    t += e0.elapsed_time(e1)
                x.grad = None
            res["%s_backward_ms%s" % (mode, "_xgrad" if xg else "")] = t / args.iters
    print(json.dumps(res))


if __name__ == "__main__":
    main()
