"""SSDN_OP_POOL_PATCH (csrc/patch_pool.hip) as an exact host model in numpy: the specification of the op (include/ssdn_hip.h states the same
in words).  Restated from that text, not from the kernel: one Philox4x32-10 block per sample, integer arithmetic for the crop origin and
the dihedral transform, numpy's "reflect" iterated to any length, one correctly rounded float32 division for the value, and the
Noise2Void selection of SSDN_OP_NOISE (tests/philox_ref.py holds Philox, u01 and n2v_pick).  Nothing here is fragile: there is no float
comparison that one ulp could turn, so the GPU tests compare every output bit for bit and exclude nothing."""
import numpy as np

from philox_ref import NS_COORD, _draw, n2v_pick, u01

NS_CROP = 5                                   # csrc/patch_pool.hip; streams 0..4 are SSDN_OP_NOISE's


def reflect(t, n):
    """r(t, n): index t >= 0 of an axis of n >= 1 elements extended by reflection, any length (array or scalar t)"""
    t = np.asarray(t, dtype=np.int64)
    if n == 1:
        return np.zeros_like(t)
    m = t % (2 * n - 2)
    return np.where(m < n, m, 2 * n - 2 - m)


def umulhi(v, span):
    """the high 32 bits of the 64-bit product of two 32-bit values"""
    return (np.asarray(v, dtype=np.uint64) * np.uint64(span)) >> np.uint64(32)


def origin(v, n, P):
    """crop origin along an axis of n elements from a random word: umulhi(v, max(n - P, 0) + 1)"""
    return umulhi(v, max(n - P, 0) + 1).astype(np.int64)


def draws(b, rows, cols, P, augment, seed, offset):
    """sample b -> (x0, y0, d): the block of counter (b, NS_CROP, offset lo, offset hi) keyed by seed"""
    v = [int(w) for w in _draw(b, NS_CROP, seed, offset)]
    return int(origin(v[0], cols, P)), int(origin(v[1], rows, P)), (v[2] >> 29) if augment else 0


def source_grid(P, d):
    """-> (u, v) int arrays [P, P] indexed [py, px]: the un-reflected source offsets of every output position under transform d.
    (u, v) = (px, py); bit 0 swaps them, bit 1 sets u = P - 1 - u, bit 2 sets v = P - 1 - v"""
    py, px = np.meshgrid(np.arange(P), np.arange(P), indexing="ij")
    u, v = px, py
    if d & 1:
        u, v = v, u
    if d & 2:
        u = P - 1 - u
    if d & 4:
        v = P - 1 - v
    return u, v


def cut(img, P, x0, y0, d):
    """img uint8 [C, rows, cols] -> uint8 [C, P, P]: out[c, py, px] = img[c, r(y0 + v, rows), r(x0 + u, cols)]"""
    _, rows, cols = img.shape
    u, v = source_grid(P, d)
    return img[:, reflect(y0 + v, rows), reflect(x0 + u, cols)]


def pack(images):
    """images: list of uint8 [C, rows, cols] -> (pool uint8 [total], offsets int64 [N], sizes int32 [N, 2]): back to back, no padding"""
    sizes = np.array([im.shape[1:] for im in images], dtype=np.int32).reshape(len(images), 2)
    nbytes = np.array([im.size for im in images], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
    pool = np.concatenate([np.ascontiguousarray(im).reshape(-1) for im in images]) if images else np.zeros(0, dtype=np.uint8)
    return pool.astype(np.uint8), offsets, sizes


def pool_patch_model(images, index, P, augment, seed, offset, params=None, n2v_box=0, n2v_radius=2):
    """SSDN_OP_POOL_PATCH for the samples `index` (image numbers) -> dict: noisy, ref float32 [B,C,P,P]; coords int64 [B, cells, 2] (None
    without n2v_box); param float32 [B, C] (None without params); origin int32 [B, 3] = (x0, y0, d); src [B, cells, 2] = the drawn (rx, ry)."""
    B, C = len(index), images[0].shape[0]
    ref = np.zeros((B, C, P, P), dtype=np.float32)
    org = np.zeros((B, 3), dtype=np.int32)
    for b, i in enumerate(index):
        img = images[int(i)]
        x0, y0, d = draws(b, img.shape[1], img.shape[2], P, augment, seed, offset)
        org[b] = (x0, y0, d)
        ref[b] = cut(img, P, x0, y0, d).astype(np.float32) / np.float32(255)
    noisy, coords, src = ref.copy(), None, None
    if n2v_box > 0:
        box, n1 = n2v_box, P // n2v_box
        coords, src = np.zeros((B, n1 * n1, 2), dtype=np.int64), np.zeros((B, n1 * n1, 2), dtype=np.int64)
        for b in range(B):
            for i in range(n1):
                for j in range(n1):
                    cell = i * n1 + j
                    w = [int(v) for v in _draw(b * n1 * n1 + cell, NS_COORD, seed, offset)]
                    c0 = min(i * box + int(u01(w[0]) * np.float32(box)), i * box + box - 1)
                    c1 = min(j * box + int(u01(w[1]) * np.float32(box)), j * box + box - 1)
                    rx, ry = int(n2v_pick(c0, n2v_radius, P, u01(w[2]))), int(n2v_pick(c1, n2v_radius, P, u01(w[3])))
                    coords[b, cell], src[b, cell] = (c0, c1), (rx, ry)
                    noisy[b, :, c1, c0] = ref[b, :, ry, rx]           # (c0, rx along the last axis, as SSDN_OP_NOISE's)
    par = None
    if params is not None:
        par = np.repeat(np.asarray(params, dtype=np.float32)[np.asarray(index, dtype=np.int64)][:, None], C, 1)
    return dict(noisy=noisy, ref=ref, coords=coords, param=par, origin=org, src=src)


# ---- the cases of the GPU test (tests/test_hip_patch_pool.py) --------------------------------------------------------------------------
SIZES = [(1, 1), (1, 7), (5, 3), (8, 8), (9, 8), (31, 33), (40, 70)]          # (rows, cols): packed back to back, odd offsets on purpose
SEED, OFFSETS = (5 << 32) | 7, ((3 << 32) | 9, 2)
INDEXES = ([0, 1, 2, 3, 3], [4, 5, 6, 6, 0], [6, 2, 5, 1, 4])                   # repeats, and every image across the calls


def case_images(C, seed=0):
    rs = np.random.RandomState(77 + 10 * seed + C)
    return [rs.randint(0, 256, (C, r, c)).astype(np.uint8) for r, c in SIZES]
