"""Gradient accumulation over micro-batches -- a measurement aid, not a test.

BASELINE config 2 (ssdn gauss25 sigma_known, blind-spot RGB, batch 32 at 64x64): optimiser steps of K micro-batches
(`Denoiser.accumulate_step` x (K - 1) + `Denoiser.train_step`), K in {1, 2, 4}, the variants alternated in blocks inside ONE process,
device events around whole blocks of groups: ms per micro-batch and per optimiser step.

usage: python tools/accum_bench.py [--steps 200] [--block 20] [--warmup 10] [--out FILE.json]
       python tools/accum_bench.py --only 1|2|4|add [--steps N]
--only runs ONE variant without events, for a kernel trace of its own (rocprofv3 --kernel-trace --stats -- python tools/accum_bench.py
--only add): "add" never steps the optimiser, so every reduction launch after the first pass carries accumulate = 1; "1" is the plain
step (accumulate = 0 in every launch).  The difference of the k_wreduce_multi averages of those two traces is the cost of the adding
epilogue."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "selfsupervised-denoising_amd"), ROOT]
import torch  # noqa: E402
import ssdn  # noqa: E402
from ssdn.datasets import NoisyDataset  # noqa: E402
from ssdn.denoiser import Denoiser  # noqa: E402
from ssdn.params import ConfigValue, NoiseAlgorithm, NoiseValue  # noqa: E402

B, P, LR = 32, 64, 3e-4


def make():
    cfg = ssdn.cfg.base()
    cfg[ConfigValue.ALGORITHM] = NoiseAlgorithm.SELFSUPERVISED_DENOISING
    cfg[ConfigValue.NOISE_STYLE] = "gauss25"
    cfg[ConfigValue.NOISE_VALUE] = NoiseValue.KNOWN
    ssdn.cfg.infer(cfg, model_only=True)
    torch.manual_seed(0)
    d = Denoiser(cfg, device="cuda:0")
    d.train()
    return d


def batches(n=4):
    MD = NoisyDataset.Metadata
    g = torch.Generator().manual_seed(1)
    out = []
    for _ in range(n):
        clean = torch.rand(B, 3, P, P, generator=g)
        noisy = torch.clamp(clean + torch.randn(B, 3, P, P, generator=g) * (25 / 255.0), 0, 1)
        out.append([noisy.cuda(), None, {MD.INPUT_NOISE_VALUES: torch.full((B, 1, 1, 1), 25 / 255.0).cuda(), MD.CLEAN: clean.cuda()}])
    return out


def group(d, data, k, i):
    """one optimiser step over k micro-batches"""
    for j in range(k - 1):
        d.accumulate_step(data[(i + j) % len(data)])
    d.train_step(data[(i + k - 1) % len(data)], LR)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="optimiser steps per variant after the warm-up")
    ap.add_argument("--block", type=int, default=20, help="optimiser steps of one variant between two switches")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--only", choices=["1", "2", "4", "add"])
    ap.add_argument("--out")
    a = ap.parse_args()
    d, data = make(), batches()
    if a.only:
        if a.only == "add":
            for i in range(a.steps):
                d.accumulate_step(data[i % len(data)])
        else:
            for i in range(a.steps):
                group(d, data, int(a.only), i)
        torch.cuda.synchronize()
        print(json.dumps({"only": a.only, "passes": a.steps * (1 if a.only == "add" else int(a.only))}))
        return
    ks = (1, 2, 4)
    for k in ks:
        for i in range(a.warmup):
            group(d, data, k, i)
    torch.cuda.synchronize()
    ms = {k: [] for k in ks}
    for r in range(-(-a.steps // a.block)):
        for k in ks if r % 2 == 0 else ks[::-1]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(a.block):
                group(d, data, k, i)
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.block)
    res = {"config": "ssdn gauss25 sigma_known RGB blind-spot, batch %d, %dx%d" % (B, P, P), "steps_per_variant": len(ms[1]) * a.block, "variants": {}}
    for k in ks:
        v = sorted(ms[k])
        med = v[len(v) // 2]
        res["variants"]["K=%d" % k] = {"ms_per_optimiser_step": round(med, 4), "ms_per_micro_batch": round(med / k, 4),
                                       "min": round(v[0], 4), "max": round(v[-1], 4), "blocks": len(v)}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
