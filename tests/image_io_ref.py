"""A numpy model of SSDN_OP_IMAGE_IN / SSDN_OP_IMAGE_OUT written from their definition in include/ssdn_hip.h (it calls neither np.pad nor
tensor2image), the package's host route the two ops replace, and the extents the image tests run on.

Layouts: an image is upright uint8 [h, w, C]; a tensor carries the image's x on axis 2 and its y on axis 3, so the un-padded extent of
image b on the tensor's axes 2 and 3 is ext[b] = (e1, e2) = (w_b, h_b)."""
import numpy as np
import torch

# extents (e1, e2) = (w, h) of the six images of a packed batch: one pixel; two (the shortest axis `reflect` has a period for); odd sizes;
# an axis of one next to a long one; the whole 64 x 64 tensor; one short of it
EXTENTS = [(1, 1), (2, 2), (5, 37), (33, 1), (64, 64), (63, 64)]
# padded tensor shapes (H, W): one workgroup tile of 32 x 64 per sample would be 32 x 64 -- these take two tiles along axis 2, and along
# axis 3 one full tile and a half-filled one
PADDED = [(64, 64), (32, 96)]
GUARD = 16                      # guard bytes between the images of a packed buffer
GUARD_BYTE = 0xAB


def fits(ext, H, W):
    """the extents of EXTENTS that fit a padded tensor of H x W"""
    return [(e1, e2) for e1, e2 in ext if e1 <= H and e2 <= W]


def reflect(k, n):
    """numpy's "reflect" continuation of an axis of n elements, for index arrays k >= 0"""
    k = np.asarray(k, dtype=np.int64)
    if n == 1:
        return np.zeros_like(k)
    p = 2 * (n - 1)
    m = k % p
    return np.where(m < n, m, p - m)


def image_in_ref(src, src_bytes, offs, ext, C, H, W):
    """src: uint8 [>= src_bytes]; offs [B]; ext [B][2] -> float32 [B,C,H,W]"""
    src = np.asarray(src, dtype=np.uint8)
    B = len(offs)
    dst = np.zeros((B, C, H, W), dtype=np.float32)
    i, j, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(C), indexing="ij")
    for b in range(B):
        e1, e2 = min(max(int(ext[b][0]), 0), H), min(max(int(ext[b][1]), 0), W)
        if e1 == 0 or e2 == 0:
            continue
        idx = (reflect(j, e2) * e1 + reflect(i, e1)) * C + c
        pos = int(offs[b]) + idx
        ok = (int(offs[b]) >= 0) & (pos < src_bytes)
        val = np.where(ok, src[np.where(ok, pos, 0)], 0).astype(np.float32) / np.float32(255.0)
        dst[b] = val.transpose(2, 0, 1)
    return dst


def quantise(v):
    """q(v) = (uint8) trunc(fl32(min(max(v, 0), 1) * 255)), q(NaN) = 0"""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        v = np.where(v > 0, v, np.float32(0))       # (NaN and -0.0 end here)
        v = np.where(v < 1, v, np.float32(1))
        return np.trunc(v * np.float32(255.0)).astype(np.int64).astype(np.uint8)


def image_out_ref(x, ext, offs, dst, dst_bytes):
    """x: float32 [B,C,H,W]; dst: uint8 buffer, changed in place and returned"""
    x = np.asarray(x, dtype=np.float32)
    B, C, H, W = x.shape
    for b in range(B):
        e1, e2 = min(max(int(ext[b][0]), 0), H), min(max(int(ext[b][1]), 0), W)
        q = quantise(x[b, :, :e1, :e2])                          # [C, x, y]
        xx, yy, cc = np.meshgrid(np.arange(e1), np.arange(e2), np.arange(C), indexing="ij")
        pos = int(offs[b]) + (yy * e1 + xx) * C + cc
        ok = (int(offs[b]) >= 0) & (pos < dst_bytes)
        dst[pos[ok]] = q.transpose(1, 2, 0)[ok]
    return dst


def make_images(ext, C, seed):
    """one upright uint8 image [h, w, C] of random bytes per extent (w, h)"""
    g = np.random.default_rng(seed)
    return [g.integers(0, 256, size=(e2, e1, C), dtype=np.uint8) for e1, e2 in ext]


def pack(images, guard=GUARD, fill=GUARD_BYTE):
    """-> (uint8 buffer: guard, image 0, guard, image 1, ..., guard; offs)"""
    parts, offs, pos = [], [], 0
    for im in images:
        parts.append(np.full(guard, fill, dtype=np.uint8))
        pos += guard
        offs.append(pos)
        parts.append(np.ascontiguousarray(im).reshape(-1))
        pos += im.size
    parts.append(np.full(guard, fill, dtype=np.uint8))
    return np.concatenate(parts), offs


def host_in(images, H, W):
    """the package's host route in: to_tensor, permute, NoisyDataset.pad_to_output_size to [C, H, W], stacked -> float32 tensor [B,C,H,W]"""
    from PIL import Image
    from ssdn.datasets import NoisyDataset
    from ssdn.datasets.transforms import to_tensor
    nd = NoisyDataset(None, "gauss25", None)
    nd.pad_uniform, nd._max_image_size = True, torch.tensor([images[0].shape[2], H, W])      # (the padded shape is the caller's)
    return torch.stack([nd.pad_to_output_size(to_tensor(Image.fromarray(im[:, :, 0] if im.shape[2] == 1 else im)).permute(0, 2, 1))
                        for im in images])


def host_out(x, images):
    """the package's host route out: NoisyDataset.unpad, tensor2image -> uint8 arrays [h, w, C]"""
    from ssdn.datasets import NoisyDataset
    from ssdn.utils import tensor2image
    shapes = torch.tensor([[im.shape[2], im.shape[1], im.shape[0]] for im in images])
    meta = {NoisyDataset.Metadata.IMAGE_SHAPE: shapes}
    x = torch.as_tensor(x)
    res = []
    for b, im in enumerate(images):
        a = np.asarray(tensor2image(NoisyDataset.unpad(x, meta, b)))
        res.append(a[:, :, None] if a.ndim == 2 else a)
    return res
