"""A numpy model of SSDN_OP_TILE_IN / SSDN_OP_TILE_OUT written from the tiling's definition in include/ssdn_hip.h: the grid of tiles, the
tiles of an image, and the blend of the tiles' values back into one image in float32.  It calls neither np.pad nor the package.

Layouts: an image is upright uint8 [h, w, C]; a tile is float32 [C, T, T] with the image's x on axis 1 and its y on axis 2 (the package's
swapped axes); the store is [Kx Ky, C, T, T], tile k = ky Kx + kx."""
import numpy as np

# (T, O) of the grid properties and of the identity tests; the GPU tests take the three of GPU_GRIDS
GRIDS = [(32, 0), (64, 0), (64, 32), (96, 32), (128, 64)]
GPU_GRIDS = [(32, 0), (64, 32), (96, 32)]
# image sizes (h, w): both axes tiled with ragged ends; one axis in one tile and the other just past a tile; one pixel past a tile; a long
# thin picture whose short axis needs a reflection longer than itself ...
SIZES = [(70, 100), (33, 129), (65, 64), (200, 37)]
# ... and for the ops also exactly one tile (T = 64) and one pixel (pads of any length, r(k, 1) = 0)
GPU_SIZES = [(70, 100), (33, 129), (64, 64), (65, 64), (200, 37), (1, 1)]


def check(T, O):
    if T < 32 or T % 32:
        raise ValueError("T must be a positive multiple of 32")
    if O < 0 or O % 32 or 2 * O > T:
        raise ValueError("O must be a multiple of 32 with 0 <= 2 O <= T")


def count(n, T, O):
    """K(n): the tiles along an axis of n elements"""
    check(T, O)
    return 1 if n <= T else -(-(n - O) // (T - O))


def origins(n, T, O):
    return [k * (T - O) for k in range(count(n, T, O))]


def reflect(k, n):
    """r(k, n) for index arrays k >= 0: numpy's "reflect" continuation of an axis of n elements, any pad length, r(k, 1) = 0"""
    k = np.asarray(k, dtype=np.int64)
    if n == 1:
        return np.zeros_like(k)
    p = 2 * (n - 1)
    m = k % p
    return np.where(m < n, m, p - m)


def weight(d, O):
    """t = fl32((float)(2 d + 1) / (float)(2 O))"""
    return (np.asarray(2 * np.asarray(d, dtype=np.int64) + 1).astype(np.float32) / np.float32(2 * O)).astype(np.float32)


def cover(n, T, O):
    """per position p < n of an axis -> (two [n] bool, ka, la, kb, lb, t): tile and local index of the lower-numbered tile a and of tile b
    (a == b where one tile covers p), and the blend weight (0 where single)"""
    S, K = T - O, count(n, T, O)
    p = np.arange(n, dtype=np.int64)
    kb = np.minimum(p // S, K - 1)
    d = p - kb * S
    two = (kb >= 1) & (d < O)
    ka, la = np.where(two, kb - 1, kb), np.where(two, d + S, d)
    t = np.where(two, weight(d, max(O, 1)), np.float32(0)).astype(np.float32)
    return two, ka, la, kb, d, t


def tile_in_ref(img, T, O, k0=0, B=None):
    """img: uint8 [h, w, C] -> float32 [B, C, T, T]: dst[b,c,i,j] = (float)img[r(oy + j, h), r(ox + i, w), c] / 255.f"""
    img = np.asarray(img, dtype=np.uint8)
    h, w, C = img.shape
    Kx, Ky = count(w, T, O), count(h, T, O)
    B = Kx * Ky - k0 if B is None else B
    assert 0 <= k0 and B >= 1 and k0 + B <= Kx * Ky
    S = T - O
    dst = np.zeros((B, C, T, T), dtype=np.float32)
    for b in range(B):
        ky, kx = divmod(k0 + b, Kx)
        xs, ys = reflect(kx * S + np.arange(T), w), reflect(ky * S + np.arange(T), h)
        dst[b] = (img[ys[None, :], xs[:, None], :].astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1)        # [i, j, c] -> [c, i, j]
    return dst


def lerp(a, b, t):
    """a + t (b - a) in float32, every operation rounded on its own"""
    a, b, t = (np.asarray(v, dtype=np.float32) for v in (a, b, t))
    with np.errstate(invalid="ignore", over="ignore"):
        return (a + (t * (b - a).astype(np.float32)).astype(np.float32)).astype(np.float32)


def blend_ref(store, w, h, T, O):
    """store: float32 [Kx Ky, C, T, T] -> float32 [C, h, w] upright: along x first for each of the one or two y-tiles, then along y; a
    position under one tile (per axis) takes that tile's value untouched"""
    store = np.asarray(store, dtype=np.float32)
    Kx, Ky = count(w, T, O), count(h, T, O)
    C = store.shape[1]
    assert store.shape == (Kx * Ky, C, T, T)
    two_x, kxa, lxa, kxb, lxb, tx = cover(w, T, O)
    two_y, kya, lya, kyb, lyb, ty = cover(h, T, O)
    cc = np.arange(C)[:, None, None]

    def along_x(ky, ly):
        """[C, h, w]: the value of y-tile ky[y] at local ly[y], interpolated along x"""
        ky, ly = ky[None, :, None], ly[None, :, None]
        a = store[ky * Kx + kxa[None, None, :], cc, lxa[None, None, :], ly]
        b = store[ky * Kx + kxb[None, None, :], cc, lxb[None, None, :], ly]
        return np.where(two_x[None, None, :], lerp(a, b, tx[None, None, :]), b)
    va, vb = along_x(kya, lya), along_x(kyb, lyb)
    return np.where(two_y[None, :, None], lerp(va, vb, ty[None, :, None]), vb).astype(np.float32)


def quantise(v):
    """SSDN_OP_IMAGE_OUT's q(v) = (uint8) trunc(fl32(min(max(v, 0), 1) * 255)), q(NaN) = 0"""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        v = np.where(v > 0, v, np.float32(0))
        v = np.where(v < 1, v, np.float32(1))
        return np.trunc(v * np.float32(255.0)).astype(np.int64).astype(np.uint8)


def tile_out_ref(store, w, h, T, O, mode):
    """mode 0 -> uint8 [h, w, C]; mode 1 -> float32 [C, h, w]"""
    v = blend_ref(store, w, h, T, O)
    return np.ascontiguousarray(quantise(v).transpose(1, 2, 0)) if mode == 0 else v


def make_image(h, w, C, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, C), dtype=np.uint8)


def make_store(n, C, T, seed):
    """random tile values with everything the blend and q must survive: negatives, values above 1, +-inf, NaN, k / 255 and its neighbours"""
    g = np.random.default_rng(seed)
    s = g.uniform(-0.3, 1.3, size=(n, C, T, T)).astype(np.float32)
    flat = s.reshape(-1)
    k = g.integers(0, 256, size=flat.size).astype(np.float32) / np.float32(255.0)
    pick = g.integers(0, 16, size=flat.size)
    flat[pick == 0] = k[pick == 0]
    flat[pick == 1] = np.nextafter(k[pick == 1], np.float32(2))
    flat[pick == 2] = np.nextafter(k[pick == 2], np.float32(-1))
    rare = g.integers(0, 400, size=flat.size)
    flat[rare == 0], flat[rare == 1], flat[rare == 2] = np.inf, -np.inf, np.nan
    return s
