"""A numpy model of SSDN_OP_NOISE_EST written from its definition in include/ssdn_hip.h: loops over the nine taps, np.add.at for the table,
Python floats (IEEE doubles, one rounding per operation) for everything after it.  It uses nothing of the package.  Also the extents and
the synthetic picture the noise-estimation tests run on.

Layouts: an image is upright uint8 [h, w, C]; ext[b] = (w_b, h_b), the image's extent on the engine's tensor axes 2 and 3, so the op clamps
w_b to H and h_b to W."""
import math

import numpy as np

NCLS, NBIN, NMIN, NEST = 8, 1024, 256, 20
C_MED = 6 * 0.6744897501960817
SIGMA_FLOOR, LAMBDA_CAP = 0.5, 260100.0
K = ((1, -2, 1), (-2, 4, -2), (1, -2, 1))
TILE_X, TILE_Y = 64, 32             # k_noise_est's tile of window centres in image space
# (h, w) of the seven images of a packed batch: no window at all (1x1, 2x2), exactly one per channel, odd sizes, one tile, a tile's edge
# inside the image in both directions, several tiles
SIZES = [(1, 1), (2, 2), (3, 3), (5, 37), (64, 64), (63, 65), (130, 70)]
# and seven around the tile: tile + 1, tile + 2 and 2 tile + 1 along x (w) and along y (h) -- the 3x3 halo crosses the tile's edge there
SIZES_TILE = [(5, TILE_X + 1), (40, TILE_X + 2), (33, 2 * TILE_X + 1), (TILE_Y + 1, 7), (TILE_Y + 2, 40), (2 * TILE_Y + 1, 66),
              (2 * TILE_Y + 1, 2 * TILE_X + 1)]
GUARD, GUARD_BYTE = 16, 0xAB
NAN = float("nan")


def table(p):
    """p: int array [h, w, C] of the bytes, -1 where a byte is not there -> (hist int64 [8,1024], ssum int64 [8])"""
    p = np.asarray(p, dtype=np.int64)
    h, w, C = p.shape
    hist, ssum = np.zeros((NCLS, NBIN), dtype=np.int64), np.zeros(NCLS, dtype=np.int64)
    if h < 3 or w < 3:
        return hist, ssum
    r = np.zeros((h - 2, w - 2, C), dtype=np.int64)
    S = np.zeros_like(r)
    valid = np.ones(r.shape, dtype=bool)
    for dy in range(3):
        for dx in range(3):
            v = p[dy:dy + h - 2, dx:dx + w - 2]
            r += K[dy][dx] * v
            S += v
            valid &= (v >= 1) & (v <= 254)
    g = (S[valid] // 9) >> 5
    k = np.minimum(np.abs(r[valid]), NBIN - 1)
    np.add.at(hist, (g, k), 1)
    np.add.at(ssum, g, S[valid])
    return hist, ssum


def grouped_median(q):
    q = [int(v) for v in q]
    N = sum(q)
    if N == 0:
        return NAN
    cum = 0
    for k, v in enumerate(q):
        if 2 * (cum + v) >= N:
            break
        cum += v
    if k == NBIN - 1:
        return NAN
    half = N / 2
    lo, hi = max(k - 0.5, 0.0), k + 0.5
    return lo + (hi - lo) * (half - cum) / q[k]


def estimates(hist, ssum):
    """-> dict(sigma, lambda, n, classes_used, nlf_sigma [8], nlf_mean [8]) as Python floats / ints / lists"""
    ng = [int(v) for v in hist.sum(1)]
    n = sum(ng)
    sigma = NAN
    if n >= NMIN:
        sigma = grouped_median(hist.sum(0)) / C_MED
        sigma = SIGMA_FLOOR if sigma < SIGMA_FLOOR else sigma
    sg, mg, num, den, used = [NAN] * NCLS, [NAN] * NCLS, 0.0, 0.0, 0
    for g in range(NCLS):
        if ng[g] >= NMIN:
            sg[g] = grouped_median(hist[g]) / C_MED
            mg[g] = int(ssum[g]) / (9.0 * ng[g])
            nm = ng[g] * mg[g]
            num = num + nm * mg[g]
            den = den + nm * (sg[g] * sg[g])
            used += 1
    lam = NAN
    if used:
        lam = LAMBDA_CAP if den == 0.0 else 255.0 * num / den
        lam = LAMBDA_CAP if lam > LAMBDA_CAP else lam
    return dict(sigma=sigma, n=n, classes_used=used, nlf_sigma=sg, nlf_mean=mg, **{"lambda": lam})


def estimate(image):
    """the whole definition for one upright uint8 image [h, w] or [h, w, C] -> (hist, ssum, estimates)"""
    a = np.asarray(image)
    hist, ssum = table(a[:, :, None] if a.ndim == 2 else a)
    return hist, ssum, estimates(hist, ssum)


def est_row(e):
    """the 20 doubles the op writes per sample"""
    return np.array([e["sigma"], e["lambda"], e["n"], e["classes_used"]] + e["nlf_sigma"] + e["nlf_mean"], dtype=np.float64)


def param(e, kind):
    """the fp32 value in the head's units: kind 0 gauss -> sigma / 255, 1 poisson -> lambda"""
    return np.float32(e["sigma"] / 255.0) if kind == 0 else np.float32(e["lambda"])


def noise_est_ref(src, src_bytes, offs, ext, C, H, W):
    """the op on a packed buffer with tables that may be wrong: ext is clamped to the tensor, a byte outside [0, src_bytes) is not there
    (so no window that holds it counts) -> (hist [B,8,1024] uint32, ssum [B,8] uint64, est [B,20] float64, list of estimate dicts)"""
    src = np.asarray(src, dtype=np.uint8)
    B = len(offs)
    hist, ssum = np.zeros((B, NCLS, NBIN), dtype=np.uint32), np.zeros((B, NCLS), dtype=np.uint64)
    est, dicts = np.zeros((B, NEST), dtype=np.float64), []
    for b in range(B):
        w, h = min(max(int(ext[b][0]), 0), H), min(max(int(ext[b][1]), 0), W)
        off = int(offs[b])
        pos = off + np.arange(h * w * C, dtype=np.int64).reshape(h, w, C)
        ok = (pos < src_bytes) if 0 <= off < src_bytes else np.zeros(pos.shape, dtype=bool)
        p = np.where(ok, src[np.where(ok, pos, 0)].astype(np.int64), -1)
        hb, sb = table(p)
        e = estimates(hb, sb)
        hist[b], ssum[b], est[b] = hb, sb, est_row(e)
        dicts.append(e)
    return hist, ssum, est, dicts


def make_images(sizes, C, seed, sigma=12.0):
    """one upright uint8 image [h, w, C] per (h, w): a ramp with Gaussian noise, so that windows spread over classes and bins and some bytes
    clip at 0 and 255"""
    g = np.random.default_rng(seed)
    res = []
    for h, w in sizes:
        y, x = np.mgrid[0:h, 0:w]
        base = 20.0 + 230.0 * ((x + 2 * y) % 97) / 96.0
        v = base[:, :, None] + g.normal(0, sigma, (h, w, C))
        res.append(np.clip(np.rint(v), 0, 255).astype(np.uint8))
    return res


def pack(images, guard=GUARD, fill=GUARD_BYTE, tail=0):
    """-> (uint8 buffer: guard, image 0, guard, image 1, ..., guard, tail; offs)"""
    parts, offs, pos = [], [], 0
    for im in images:
        parts.append(np.full(guard, fill, dtype=np.uint8))
        pos += guard
        offs.append(pos)
        parts.append(np.ascontiguousarray(im).reshape(-1))
        pos += im.size
    parts.append(np.full(guard + tail, fill, dtype=np.uint8))
    return np.concatenate(parts), offs


def synthetic(h=256, w=384, texture=0.0):
    """the clean synthetic picture of DESIGN.md section 3.17, float64 [h, w, 3] in [0, 1]"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = 0.5 + 0.35 * np.sin(x / 37) * np.cos(y / 53) + 0.1 * np.sin((x + y) / 11)
    img = np.stack([base, np.roll(base, 17, 0), np.roll(base, 29, 1)], -1)
    img[h // 3:h // 2, w // 4:w // 2] *= 0.4
    img = img + (texture * np.sin(x / 1.3) * np.sin(y / 1.7))[:, :, None]
    return np.clip(img, 0, 1)


def add_noise(clean, kind, value, seed):
    """gauss: N(0, (value/255)^2); poisson: TRUE Poisson noise rng.poisson(value x) / value (not the package's add_poisson, whose rate-1
    quirk has a variance that does not depend on the intensity) -> uint8, clipped and quantised as np.uint8(v * 255)"""
    rng = np.random.default_rng(seed)
    v = clean + rng.normal(0, value / 255.0, clean.shape) if kind == "gauss" else rng.poisson(value * clean) / value
    return np.uint8(np.clip(v, 0, 1) * 255)


def close(a, b, rel=1e-12):
    """floats equal to `rel` relative, NaN equal to NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all((np.isnan(a) & np.isnan(b)) | (np.abs(a - b) <= rel * np.abs(b))))
