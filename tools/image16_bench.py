"""The 16-bit image and tile ops beside their byte siblings -- a measurement aid, not a test.

One mono image of --size x --size on the device; per op `--launches` back-to-back launches between two events after `--warmup`, `--rounds`
rounds in which the byte op and the 16-bit op alternate; prints per op the per-launch medians in microseconds and their ratio.
IMAGE_IN / IMAGE_OUT: the image as one sample of a [1, 1, size, size] batch.  TILE_IN / TILE_OUT: all its tiles at --tile / --overlap.

usage: python tools/image16_bench.py [--size 2048] [--tile 512] [--overlap 128] [--launches 50] [--warmup 10] [--rounds 5] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "selfsupervised-denoising_amd"), ROOT]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from ssdn.hip import lib as L  # noqa: E402
from ssdn.hip.engine import OpList, current_stream  # noqa: E402


def timed(ops, launches, warmup):
    """microseconds per launch of a one-op list"""
    s = current_stream()
    for _ in range(warmup):
        ops.run(s)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        ops.run(s)
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=128)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, T, O = a.size, a.tile, a.overlap
    K = L.tile_count(n, T, O)
    g = np.random.default_rng(0)
    img8 = torch.from_numpy(g.integers(0, 256, size=n * n, dtype=np.uint8)).to(dev)
    img16 = torch.from_numpy(g.integers(0, 65536, size=n * n).astype(np.uint16)).to(dev)
    out8, out16 = torch.zeros_like(img8), torch.zeros_like(img16)
    offs = torch.zeros(1, dtype=torch.int64, device=dev)
    ext = torch.tensor([n, n], dtype=torch.int32, device=dev)
    planes = torch.rand((1, 1, n, n), dtype=torch.float32, device=dev)
    tiles = torch.rand((K * K, 1, T, T), dtype=torch.float32, device=dev)
    p = lambda t: t.data_ptr()      # noqa: E731
    ops = {
        "image_in": (OpList([("image_in", L.ImageInArgs(p(img8), n * n, p(offs), p(ext), 1, 1, n, n, p(planes)))]),
                     OpList([("image_in16", L.ImageIn16Args(p(img16), n * n, p(offs), p(ext), 1, 1, n, n, 65535, p(planes)))])),
        "image_out": (OpList([("image_out", L.ImageOutArgs(p(planes), p(ext), p(offs), p(out8), n * n, 1, 1, n, n))]),
                      OpList([("image_out16", L.ImageOut16Args(p(planes), p(ext), p(offs), p(out16), n * n, 1, 1, n, n, 65535))])),
        "tile_in": (OpList([("tile_in", L.TileInArgs(p(img8), n * n, n, n, 1, T, O, K, K, 0, K * K, p(tiles)))]),
                    OpList([("tile_in16", L.TileIn16Args(p(img16), n * n, n, n, 1, T, O, K, K, 0, K * K, 65535, p(tiles)))])),
        "tile_out": (OpList([("tile_out", L.TileOutArgs(p(tiles), n, n, 1, T, O, K, K, 0, p(out8), n * n))]),
                     OpList([("tile_out16", L.TileOut16Args(p(tiles), n, n, 1, T, O, K, K, 65535, p(out16), n * n))])),
    }
    lines = ["%s, one mono image of %d x %d, tiles of %d overlapping by %d (%d tiles); us per launch, median of %d rounds of %d launches, "
             "byte op and 16-bit op alternating" % (torch.cuda.get_device_name(0), n, n, T, O, K * K, a.rounds, a.launches)]
    for name in ("image_in", "image_out", "tile_in", "tile_out"):
        o8, o16 = ops[name]
        t8, t16 = [], []
        for _ in range(a.rounds):
            t8.append(timed(o8, a.launches, a.warmup))
            t16.append(timed(o16, a.launches, a.warmup))
        m8, m16 = float(np.median(t8)), float(np.median(t16))
        lines.append("%-9s 8-bit %8.2f  16-bit %8.2f  ratio %.3f   (8-bit runs %s; 16-bit runs %s)"
                     % (name, m8, m16, m16 / m8, " ".join("%.2f" % v for v in t8), " ".join("%.2f" % v for v in t16)))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
