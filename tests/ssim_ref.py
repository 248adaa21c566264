"""An SSIM that shares no code with the package: float64 numpy with scipy.ndimage.correlate1d (Wang, Bovik, Sheikh, Simoncelli 2004: an
11 x 11 separable Gaussian window of sd 1.5 at the positions where it lies wholly inside the image, C1 = 0.01^2, C2 = 0.03^2, data range 1,
population covariance), and the image pairs the SSIM tests run on."""
import numpy as np
import torch
from scipy.ndimage import correlate1d

WIN = 11


def window():
    k = np.arange(WIN, dtype=np.float64) - WIN // 2
    g = np.exp(-(k ** 2) / (2 * 1.5 ** 2))
    return g / g.sum()


def ssim_ref(x, ref):
    """x, ref: [B,C,H,W] (torch or numpy) -> (values [B] float64, map [B,C,H-10,W-10] float64), numpy"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    g, r = window(), WIN // 2

    def E(t):                         # the filtered image, cropped to the positions whose window saw no border
        t = correlate1d(correlate1d(t, g, axis=-1, mode="constant"), g, axis=-2, mode="constant")
        return t[..., r:t.shape[-2] - r, r:t.shape[-1] - r]
    mx, my = E(x), E(y)
    sxx, syy, sxy = E(x * x) - mx * mx, E(y * y) - my * my, E(x * y) - mx * my
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    smap = (2 * mx * my + c1) * (2 * sxy + c2) / ((mx ** 2 + my ** 2 + c1) * (sxx + syy + c2))
    return smap.reshape(smap.shape[0], -1).mean(1), smap


SDS = (1 / 255.0, 25 / 255.0)


def make_pair(B, C, H, W, seed=0):
    """(x, ref) float32 [B,C,H,W].  ref: uniform noise under a 7 x 7 box filter, with a flat 0.5 patch and a flat saturated 1.0 patch
    (12 x 12 each where the image has the room; smaller images keep the part that fits).  x: ref plus Gaussian noise of sd 1/255 (even
    samples) or 25/255 (odd samples), not clipped, so values leave [0,1]; then a region where x == ref exactly, reaching into the flat 0.5
    patch (both images constant: the variances cancel completely), and a region where x = 1 - ref (negative SSIM), reaching into the
    saturated patch."""
    rng = np.random.default_rng(1000 + seed)
    u = rng.random((B, C, H + 6, W + 6))
    box = np.ones(7) / 7
    ref = correlate1d(correlate1d(u, box, axis=-1, mode="constant"), box, axis=-2, mode="constant")[..., 3:H + 3, 3:W + 3]
    ref[..., 2:14, 2:14] = 0.5
    ref[..., 2:14, 16:28] = 1.0
    ref = ref.astype(np.float32)
    x = ref.astype(np.float64)
    for b in range(B):
        x[b] += SDS[b % 2] * rng.standard_normal((C, H, W))
    x = x.astype(np.float32)
    x[..., 8:30, 2:16] = ref[..., 8:30, 2:16]
    x[..., 8:30, 18:32] = np.float32(1) - ref[..., 8:30, 18:32]
    return torch.from_numpy(x), torch.from_numpy(ref)
