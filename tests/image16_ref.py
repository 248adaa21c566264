"""A numpy model of the five 16-bit ops -- SSDN_OP_IMAGE_IN16 / IMAGE_OUT16 / TILE_IN16 / TILE_OUT16 / POOL_PATCH16 -- written from their
definition in include/ssdn_hip.h.  The sample model is stated here once; the index arithmetic (reflect, the tiling, the blend, the Philox
draws) is that of the byte ops' models (image_io_ref.py, tile_ref.py, patch_pool_ref.py), whose helpers this file calls.  It imports nothing
of the package.

Layouts are the siblings': an image is upright uint16 [h, w, C]; a tensor carries the image's x on axis 2 and its y on axis 3; a pool
image is planar uint16 [C, rows, cols].  Counts and offsets are in SAMPLES."""
import numpy as np

import image_io_ref as IO
import patch_pool_ref as PP
import tile_ref as TR

WHITES = (65535, 4095)          # the white levels of the GPU tests: the full range, and a 12-bit camera file in a 16-bit container
GUARD = 16                      # guard samples between the images of a packed buffer
GUARD_SAMPLE = 0xABCD


def sample_in(s, white):
    """value = (float)min(s, white) / (float)white: one correctly rounded float32 division; samples above white are 1.0"""
    s = np.minimum(np.asarray(s).astype(np.int64), int(white))
    return (s.astype(np.float32) / np.float32(white)).astype(np.float32)


def q16(v, white):
    """q16(v) = (uint16) rint(fl32(min(max(v, 0), 1) * (float)white)): ties to even (np.rint), q16(NaN) = 0, q16(-0.0) = 0"""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        v = np.where(v > 0, v, np.float32(0))       # (NaN and -0.0 end here)
        v = np.where(v < 1, v, np.float32(1))
        return np.rint((v * np.float32(white)).astype(np.float32)).astype(np.int64).astype(np.uint16)


def q16_truncating(v, white):
    """what q16 would be with SSDN_OP_IMAGE_OUT's truncation: the variant the definition rejects (it fails the round trip)"""
    v = np.minimum(np.maximum(np.asarray(v, dtype=np.float32), np.float32(0)), np.float32(1))
    return np.trunc((v * np.float32(white)).astype(np.float32)).astype(np.int64).astype(np.uint16)


def image_in16_ref(src, src_count, offs, ext, C, H, W, white):
    """src: uint16 [>= src_count]; offs [B] in samples; ext [B][2] -> float32 [B,C,H,W] (image_io_ref.image_in_ref with the sample model)"""
    src = np.asarray(src, dtype=np.uint16)
    B = len(offs)
    dst = np.zeros((B, C, H, W), dtype=np.float32)
    i, j, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(C), indexing="ij")
    for b in range(B):
        e1, e2 = min(max(int(ext[b][0]), 0), H), min(max(int(ext[b][1]), 0), W)
        if e1 == 0 or e2 == 0:
            continue
        idx = (IO.reflect(j, e2) * e1 + IO.reflect(i, e1)) * C + c
        off = int(offs[b])
        ok = (0 <= off < src_count) & (idx < src_count - off)
        val = sample_in(np.where(ok, src[np.where(ok, off + idx, 0)], 0), white)
        dst[b] = val.transpose(2, 0, 1)
    return dst


def image_out16_ref(x, ext, offs, dst, dst_count, white):
    """x: float32 [B,C,H,W]; dst: uint16 buffer, changed in place and returned"""
    x = np.asarray(x, dtype=np.float32)
    B, C, H, W = x.shape
    for b in range(B):
        e1, e2 = min(max(int(ext[b][0]), 0), H), min(max(int(ext[b][1]), 0), W)
        q = q16(x[b, :, :e1, :e2], white)                        # [C, x, y]
        xx, yy, cc = np.meshgrid(np.arange(e1), np.arange(e2), np.arange(C), indexing="ij")
        idx = (yy * e1 + xx) * C + cc
        off = int(offs[b])
        ok = (0 <= off < dst_count) & (idx < dst_count - off)
        dst[(off + idx)[ok]] = q.transpose(1, 2, 0)[ok]
    return dst


def tile_in16_ref(img, T, O, white, k0=0, B=None):
    """img: uint16 [h, w, C] -> float32 [B, C, T, T]: dst[b,c,i,j] = in(img[r(oy + j, h), r(ox + i, w), c])"""
    img = np.asarray(img, dtype=np.uint16)
    h, w, C = img.shape
    Kx, Ky = TR.count(w, T, O), TR.count(h, T, O)
    B = Kx * Ky - k0 if B is None else B
    assert 0 <= k0 and B >= 1 and k0 + B <= Kx * Ky
    S = T - O
    dst = np.zeros((B, C, T, T), dtype=np.float32)
    for b in range(B):
        ky, kx = divmod(k0 + b, Kx)
        xs, ys = TR.reflect(kx * S + np.arange(T), w), TR.reflect(ky * S + np.arange(T), h)
        dst[b] = sample_in(img[ys[None, :], xs[:, None], :], white).transpose(2, 0, 1)        # [i, j, c] -> [c, i, j]
    return dst


def tile_out16_ref(store, w, h, T, O, white):
    """-> uint16 [h, w, C]: q16 of SSDN_OP_TILE_OUT's blend"""
    return np.ascontiguousarray(q16(TR.blend_ref(store, w, h, T, O), white).transpose(1, 2, 0))


def pool_patch16_model(images, index, P, augment, seed, offset, white, params=None, n2v_box=0, n2v_radius=2):
    """SSDN_OP_POOL_PATCH16: the byte op's draws, crop, transform and Noise2Void selection (patch_pool_ref.pool_patch_model gives origin,
    coords, src and param -- none of them depends on a sample's value) over the sample model -> the same dict"""
    m = PP.pool_patch_model(images, index, P, augment, seed, offset, params=params, n2v_box=n2v_box, n2v_radius=n2v_radius)
    ref = np.stack([sample_in(PP.cut(images[int(i)], P, *(int(v) for v in m["origin"][b])), white) for b, i in enumerate(index)])
    noisy = ref.copy()
    if n2v_box > 0:
        for b in range(len(index)):
            for (c0, c1), (rx, ry) in zip(m["coords"][b], m["src"][b]):
                noisy[b, :, c1, c0] = ref[b, :, ry, rx]
    m["noisy"], m["ref"] = noisy, ref
    return m


def pack16(images):
    """patch_pool_ref.pack for uint16 images: (pool uint16 [total], offsets int64 [N] in samples, sizes int32 [N, 2])"""
    _, offsets, sizes = PP.pack(images)
    return np.concatenate([np.ascontiguousarray(im).reshape(-1) for im in images]).astype(np.uint16), offsets, sizes


def make_images16(ext, C, seed, white):
    """one upright uint16 image [h, w, C] per extent (w, h): samples over [0, white], and for white < 65535 a share of them above it"""
    g = np.random.default_rng(seed)
    out = []
    for e1, e2 in ext:
        im = g.integers(0, white + 1, size=(e2, e1, C)).astype(np.uint16)
        if white < 65535:
            over = g.integers(0, 8, size=im.shape) == 0
            im[over] = g.integers(white + 1, 65536, size=int(over.sum())).astype(np.uint16)
        out.append(im)
    return out


def pack_samples(images, guard=GUARD, fill=GUARD_SAMPLE):
    """image_io_ref.pack for uint16: (buffer: guard, image 0, guard, image 1, ..., guard; offs in samples)"""
    parts, offs, pos = [], [], 0
    for im in images:
        parts.append(np.full(guard, fill, dtype=np.uint16))
        pos += guard
        offs.append(pos)
        parts.append(np.ascontiguousarray(im).reshape(-1))
        pos += im.size
    parts.append(np.full(guard, fill, dtype=np.uint16))
    return np.concatenate(parts), offs


def make_store16(n, C, T, seed, white):
    """tile_ref.make_store with the quantiser's edges at this white level: k / white, its neighbours, and exact .5 ties"""
    g = np.random.default_rng(seed)
    s = TR.make_store(n, C, T, seed)
    flat = s.reshape(-1)
    k = g.integers(0, white + 1, size=flat.size).astype(np.float32) / np.float32(white)
    pick = g.integers(0, 16, size=flat.size)
    flat[pick == 3] = k[pick == 3]
    flat[pick == 4] = np.nextafter(k[pick == 4], np.float32(2))
    flat[pick == 5] = np.nextafter(k[pick == 5], np.float32(-1))
    return s


def widen(a):
    """bytes as uint16 samples of the same values"""
    return np.asarray(a, dtype=np.uint8).astype(np.uint16)
