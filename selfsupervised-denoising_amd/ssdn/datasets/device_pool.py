"""Training on images that are ALREADY noisy: a device-resident pool of the training images and the minibatch stream cut out of it.

`NoisyDataset` and `DevicePatchStream` start from a clean image and synthesise the corruption; the three pipelines that never read a clean
image in their loss (ssdn, ssdn_u_only, n2v) can train on a folder of noisy images alone.  `ImagePool` decodes every training image ONCE,
packs the bytes back to back and keeps them on the device; `DevicePoolStream` cuts every minibatch out of that pool with ONE launch
(SSDN_OP_POOL_PATCH of libssdn_hip.so: random crop, optional dihedral transform, / 255, the Noise2Void manipulation; SSDN_OP_POOL_PATCH16
with min(sample, white) / white for a 16-bit pool) that writes straight into the denoiser's input buffer.  No DataLoader, no workers, no
upload per step beyond the B image numbers.

Yields `[inp, ref, metadata]` in the contract of `DevicePatchStream` (same keys, shapes and dtypes) except that `Metadata.CLEAN` is absent:
there is no clean image.  An image smaller than the patch is extended by reflection to the right and downwards only (the host `RandomCrop`
pads both sides; crop positions are "distribution only" in this project, ssdn/datasets/transforms.py).  With CPU tensors (no GPU: tests)
the same crop arithmetic runs through torch, the random stream then being a torch generator."""
from __future__ import annotations

from typing import Dict, Iterable, Iterator, List, Optional

import torch

from ssdn.datasets.noise_wrapper import NULL_IMAGE, NoisyDataset
from ssdn.params import NoiseAlgorithm

DEFAULT_POOL_BYTES = 8 << 30          # cap of the packed pool (`--pool_gb` overrides it); an MI355X holds far more, a typo should not
POOL_ALGORITHMS = (NoiseAlgorithm.SELFSUPERVISED_DENOISING, NoiseAlgorithm.SELFSUPERVISED_DENOISING_MEAN_ONLY, NoiseAlgorithm.NOISE_TO_VOID)


class ImagePool:
    """Every image of an UNTRANSFORMED dataset (the folder or HDF5 child `DenoiserTrainer._open` returns), read once through
    `dataset[i][0]`, converted as `CleanPatches.__getitem__` converts (x 255, round, clamp, uint8), packed without padding and uploaded:
    `pool` uint8 [total], `offsets` int64 [N], `sizes` int32 [N, 2] = (rows, cols) of the dataset's own planar [C, rows, cols] tensor, and
    optionally `params` fp32 [N], the per-image noise parameter.  The host keeps `files`, the length and copies of offsets and sizes.
    In a multi-GPU job every rank holds the whole pool.
    A folder whose files are all 16-bit grey (their PIL modes, read from the headers) becomes a 16-bit pool: `bits` = 16, `pool` uint16 in
    the same planar layout, read through `ssdn.utils.load_image` (the dataset's own route clips at 255), `offsets` in SAMPLES, `nbytes` and
    the cap at 2 bytes per sample, `white` the sample value that means 1.0 (None = 65535).  Files of both depths are refused; HDF5 datasets
    are 8-bit; `white` with an 8-bit pool is refused."""

    def __init__(self, dataset, device, max_bytes: int = DEFAULT_POOL_BYTES, white: Optional[int] = None):
        if getattr(dataset, "transform", None) is not None:
            raise ValueError("ImagePool: the dataset must be untransformed (the pool holds whole images; the crop is the stream's)")
        n = len(dataset)
        if n < 1:
            raise ValueError("ImagePool: the dataset is empty")
        self._start(device, max_bytes, list(dataset.files) if hasattr(dataset, "files") else None)
        bits = 8
        if self.files is not None:                  # the headers alone tell the depth and whether the pool fits: nothing is decoded before
            bits, total = self._read_headers(int(getattr(dataset, "channels", 0)))
            if hasattr(dataset, "image_size"):
                self._check_cap(total * (bits // 8), n)
        elif hasattr(dataset, "image_size"):
            self._check_cap(sum(int(torch.prod(dataset.image_size(i, ignore_transform=True))) for i in range(n)), n)
        if bits == 16:
            from ssdn.utils.data import load_image
            swap = getattr(dataset, "output_format", "CHW") is not None      # the dataset's own relabelling (datasets/folder.py)

            def read(i):
                t = torch.from_numpy(load_image(self.files[i], dataset.channels))              # uint16 [h, w, 1]
                return (t.permute(2, 1, 0) if swap else t.permute(2, 0, 1)).contiguous()
        else:
            def read(i):
                img = dataset[i][0]
                if img.dim() != 3:
                    raise ValueError("ImagePool: image %d is not a [C, rows, cols] tensor" % i)
                return (img * 255.0).round().clamp_(0, 255).to(torch.uint8).contiguous()
        self._fill(n, read, bits, white)

    @classmethod
    def from_images(cls, images, device, max_bytes: int = DEFAULT_POOL_BYTES, white: Optional[int] = None) -> "ImagePool":
        """A pool of upright arrays or tensors [h, w] or [h, w, C], all uint8 or all uint16 -- the route for 16-bit RGB, which no PIL file
        delivers.  Image i is stored as the datasets would hand it out: planar [C, w, h] (rows run along the picture's x)."""
        import numpy as np
        ts = []
        for k, im in enumerate(images):
            t = torch.from_numpy(np.ascontiguousarray(im)) if isinstance(im, np.ndarray) else im
            if not torch.is_tensor(t) or t.dtype not in (torch.uint8, torch.uint16) or t.dim() not in (2, 3):
                raise ValueError("ImagePool: image %d is not a uint8 or uint16 array or tensor [h, w] or [h, w, C]" % k)
            ts.append((t.unsqueeze(-1) if t.dim() == 2 else t).detach().cpu())
        if not ts:
            raise ValueError("ImagePool: the dataset is empty")
        depths = {t.dtype for t in ts}
        if len(depths) != 1:
            raise ValueError("ImagePool: uint8 and uint16 images in one pool")
        self = cls.__new__(cls)
        self._start(device, max_bytes, None)
        self._fill(len(ts), lambda i: ts[i].permute(2, 1, 0).contiguous(), 16 if ts[0].dtype == torch.uint16 else 8, white)
        return self

    def _start(self, device, max_bytes: int, files: Optional[List[str]]):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.files, self.max_bytes = files, int(max_bytes)

    def _read_headers(self, channels: int):
        """-> (8 or 16, the samples of all files) from the files' headers; a folder of both depths is refused, naming a file of each"""
        from PIL import Image
        from ssdn.utils.data import image_bits
        first, total = {}, 0
        for f in self.files:
            with Image.open(f) as im:
                (w, h), b = im.size, image_bits(im.mode)
            first.setdefault(b, f)
            total += w * h * (channels or len(im.getbands()))
        if len(first) == 2:
            raise ValueError("ImagePool: 8-bit and 16-bit files in one folder (%s is 8-bit, %s is 16-bit): a pool is of one depth"
                             % (first[8], first[16]))
        return next(iter(first)), total

    def _fill(self, n: int, read, bits: int, white: Optional[int]):
        """pack read(0) .. read(n - 1), integer tensors [C, rows, cols] of `bits` bits per sample, and upload them"""
        if bits == 16:
            from ssdn.hip.engine import check_white
            white = check_white(white, "ImagePool: white")
        elif white is not None:
            raise ValueError("ImagePool: white is the white level of a 16-bit pool and these images are 8-bit")
        self.bits, self.white = bits, white
        size = bits // 8
        images, sizes, total = [], [], 0
        for i in range(n):
            img = read(i)
            if images and img.shape[0] != images[0].shape[0]:
                raise ValueError("ImagePool: image %d has %d channel(s), image 0 has %d" % (i, img.shape[0], images[0].shape[0]))
            total += img.numel() * size
            sizes.append((img.shape[1], img.shape[2]))
            if total <= self.max_bytes:
                images.append(img)
            elif len(images) > 1:
                del images[1:]                      # over the cap: only the total is still wanted (image 0 keeps the channel count)
        self._check_cap(total, n)
        self.n, self.channels, self.nbytes = n, int(images[0].shape[0]), total
        self.sizes_host = torch.tensor(sizes, dtype=torch.int32).reshape(n, 2)
        per = self.sizes_host.to(torch.int64).prod(1) * self.channels
        self.offsets_host = torch.cumsum(per, 0) - per                 # running sums in samples: no alignment padding
        host = torch.empty(total // size, dtype=images[0].dtype)
        for off, img in zip(self.offsets_host.tolist(), images):
            host[off:off + img.numel()] = img.reshape(-1)
        del images
        self.pool = host.to(self.device)
        self.offsets, self.sizes = self.offsets_host.to(self.device), self.sizes_host.to(self.device)
        self.params: Optional[torch.Tensor] = None
        self.params_host: Optional[torch.Tensor] = None

    def _check_cap(self, total: int, n: int):
        if total > self.max_bytes:
            raise ValueError("ImagePool: the %d training images need %d bytes (%.2f GiB) on the device, the cap is %d bytes (%.2f GiB): "
                             "raise it with --pool_gb (DenoiserTrainer.pool_bytes) or train on fewer images"
                             % (n, total, total / 2 ** 30, self.max_bytes, self.max_bytes / 2 ** 30))

    def __len__(self) -> int:
        return self.n

    def image(self, i: int) -> torch.Tensor:
        """image i as the pool holds it: a uint8 (16-bit pool: uint16) [C, rows, cols] view of the pool, on the pool's device"""
        rows, cols = (int(v) for v in self.sizes_host[i])
        off = int(self.offsets_host[i])
        return self.pool[off:off + self.channels * rows * cols].view(self.channels, rows, cols)

    def upright(self, i: int) -> torch.Tensor:
        """image i as `Denoiser.denoise` and `Denoiser.estimate_noise` take it: uint8 (16-bit pool: uint16) [h, w, C] on the host (the
        dataset's tensors carry the package's swapped axes: rows run along the picture's x)"""
        return self.image(i).cpu().permute(2, 1, 0).contiguous()

    def set_params(self, values) -> "ImagePool":
        """the per-image noise parameter table, fp32 [N] in the head's units"""
        v = torch.as_tensor(values, dtype=torch.float32).reshape(-1).cpu()
        if v.numel() != self.n:
            raise ValueError("ImagePool: %d noise parameters for %d images" % (v.numel(), self.n))
        self.params_host, self.params = v, v.to(self.device)
        return self

    def estimate_params(self, denoiser, kind: str, chunk: int = 64) -> "ImagePool":
        """fill the table with `Denoiser.estimate_noise`'s "noise_param" of every image (sigma / 255 for gauss, lambda for poisson)"""
        if self.bits == 16:
            from ssdn.hip.lib import NOISE_EST_BYTES_ONLY
            raise ValueError("ImagePool: " + NOISE_EST_BYTES_ONLY)
        vals: List[float] = []
        for lo in range(0, self.n, chunk):
            est = denoiser.estimate_noise([self.upright(i) for i in range(lo, min(lo + chunk, self.n))], kind=kind)
            vals += [e["noise_param"] for e in est]
        bad = [i for i, v in enumerate(vals) if not (v == v and v > 0.0)]
        if bad:
            name = self.files[bad[0]] if self.files else "image %d" % bad[0]
            raise ValueError("ImagePool: no noise level could be estimated for %d image(s), the first is %s (too small or without noise): "
                             "remove them or train with --noisy and the style's own parameter" % (len(bad), name))
        return self.set_params(vals)


def _reflect(t: torch.Tensor, n: int) -> torch.Tensor:
    """r(t, n) of SSDN_OP_POOL_PATCH: numpy's "reflect" iterated to any length"""
    if n == 1:
        return torch.zeros_like(t)
    m = t % (2 * n - 2)
    return torch.where(m < n, m, 2 * n - 2 - m)


def cut_patch(img: torch.Tensor, P: int, x0: int, y0: int, d: int) -> torch.Tensor:
    """SSDN_OP_POOL_PATCH's patch of one [C, rows, cols] image through torch indexing: out[c, py, px] = img[c, r(y0 + v), r(x0 + u)] with
    (u, v) = (px, py), bit 0 of d swapping them, bit 1 setting u = P - 1 - u, bit 2 setting v = P - 1 - v"""
    rows, cols = img.shape[1:]
    py, px = torch.meshgrid(torch.arange(P, device=img.device), torch.arange(P, device=img.device), indexing="ij")
    u, v = px, py
    if d & 1:
        u, v = v, u
    if d & 2:
        u = P - 1 - u
    if d & 4:
        v = P - 1 - v
    return img[:, _reflect(y0 + v, rows), _reflect(x0 + u, cols)]


class DevicePoolStream:
    """Minibatches `[inp, ref, metadata]` out of an `ImagePool`.  batches: an iterable of lists of image numbers (a BatchSampler over the
    trainer's sampler, or its `_RankShard`): the sampling order and its checkpoint contract stay the host's.  per_image: the noise
    parameter of a sample is its image's entry of `pool.params` (`--noisy auto`) instead of the style's number.
    Reference and coefficient: ssdn -> the null image and 0; ssdn_u_only -> inp and the input coefficient; n2v -> the unmanipulated patch
    (the textbook Noise2Void target) and the input coefficient."""

    def __init__(self, pool: ImagePool, batches: Iterable, algorithm: NoiseAlgorithm, noise_style: str, patch_size: int,
                 augment: bool = False, per_image: bool = False, seed: Optional[int] = None, rank: int = 0):
        from ssdn.utils import noise
        if algorithm not in POOL_ALGORITHMS:
            raise ValueError("device pool stream: %s needs a clean image or a second realisation; only ssdn, ssdn_u_only and n2v train on "
                             "images that are already noisy" % algorithm.value)
        if per_image and pool.params is None:
            raise ValueError("device pool stream: per-image noise parameters need ImagePool.set_params or estimate_params first")
        self.pool, self.batches, self.algorithm, self.device = pool, batches, algorithm, pool.device
        self.patch_size, self.augment, self.per_image = int(patch_size), bool(augment), bool(per_image)
        if self.patch_size < 1:
            raise ValueError("device pool stream: patch_size must be at least 1")
        kind, params, _ = noise.parse_style(noise_style)
        if kind == "impulse":
            vals = [noise.impulse_alpha(p) for p in params]
        else:
            vals = [(p / 255.0 if (kind == "gauss" and isinstance(p, int)) else float(p)) for p in params]
        self.fixed = float(vals[0]) if vals else 0.0            # the style's own number (the lower end of a range nobody reads)
        self.generator = torch.Generator(device=self.device)
        if seed is None:
            seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())      # drawn from the (checkpointed) host RNG
        self.rank = rank
        self.seed = seed + rank            # ranks never share a crop stream
        self.generator.manual_seed(self.seed)
        self._calls = 0                    # Philox counter of SSDN_OP_POOL_PATCH: a fresh offset per minibatch
        self._static: Dict = {}
        self._denoiser = None
        self.keep_origin = False           # tests: leave (x0, y0, d) of the last minibatch in `last_origin` (int32 [B, 3])
        self.last_origin: Optional[torch.Tensor] = None

    def state_dict(self) -> Dict:
        """as DevicePatchStream's: the Philox key without the rank offset, and the number of minibatches prepared so far"""
        return {"seed": int(self.seed - self.rank), "calls": int(self._calls)}

    def load_state_dict(self, sd: Dict, rank: Optional[int] = None):
        self.rank = self.rank if rank is None else rank
        self.seed = int(sd["seed"]) + self.rank
        self._calls = int(sd["calls"])
        self.generator.manual_seed(self.seed)

    def attach(self, denoiser):
        """write every minibatch straight into `denoiser`'s training input buffer; the yielded input IS that buffer"""
        self._denoiser = denoiser
        return self

    def __len__(self) -> int:
        return len(self.batches)

    def __iter__(self) -> Iterator:
        for indexes in self.batches:
            yield self.prepare(indexes)

    # ---- one minibatch --------------------------------------------------------------------------------------------------------
    def _indexes(self, indexes) -> torch.Tensor:
        idx = torch.as_tensor(list(indexes) if not torch.is_tensor(indexes) else indexes, dtype=torch.int64).reshape(-1).cpu()
        if idx.numel() < 1:
            raise ValueError("device pool stream: an empty minibatch")
        if int(idx.min()) < 0 or int(idx.max()) >= self.pool.n:          # the kernel trusts them: checked before upload
            raise IndexError("device pool stream: image numbers must lie in [0, %d)" % self.pool.n)
        return idx

    def _statics(self, B: int) -> Dict:
        st = self._static.get(B)
        if st is None:
            Cn, P = self.pool.channels, self.patch_size
            st = {"shape": torch.tensor([Cn, P, P]).repeat(B, 1), "null": torch.stack([NULL_IMAGE] * B).to(self.device)}
            self._static = {B: st}
        return st

    def _coeff(self, st: Dict, B: int, value: float) -> torch.Tensor:
        k = ("coeff", value)
        if k not in st:
            st[k] = torch.full((B, 1, 1, 1), float(value), dtype=torch.float32, device=self.device)
            st[k]._ssdn_const = True        # never rewritten: Denoiser uploads this very object once (denoiser.py, KNOWN sigma)
        return st[k]

    def _batch(self, idx: torch.Tensor, inp: torch.Tensor, plain: Optional[torch.Tensor], par: Optional[torch.Tensor],
               coords: Optional[torch.Tensor]) -> List:
        MD, B = NoisyDataset.Metadata, idx.numel()
        st = self._statics(B)
        if par is not None:
            par._ssdn_per_sample = True     # one value per sample repeated over the channels: the head takes channel 0's
        inp_c = par if par is not None else self._coeff(st, B, self.fixed)
        metadata: Dict = {}
        if coords is not None:
            metadata[MD.MASK_COORDS] = coords
        if self.algorithm == NoiseAlgorithm.SELFSUPERVISED_DENOISING:
            ref, ref_c = st["null"], self._coeff(st, B, 0)
        elif self.algorithm == NoiseAlgorithm.SELFSUPERVISED_DENOISING_MEAN_ONLY:
            ref, ref_c = inp, inp_c
        else:
            ref, ref_c = plain, inp_c
        metadata[MD.INDEXES] = idx
        metadata[MD.IMAGE_SHAPE] = st["shape"]
        metadata[MD.INPUT_NOISE_VALUES] = inp_c
        metadata[MD.REFERENCE_NOISE_VALUES] = ref_c
        return [inp, ref, metadata]

    def prepare(self, indexes):
        idx = self._indexes(indexes)
        if self.device.type == "cuda":
            return self._prepare_hip(idx)
        return self._prepare_torch(idx)

    def _prepare_hip(self, idx: torch.Tensor):
        import ctypes as C
        from ssdn.hip import lib as L
        from ssdn.utils import n2v_ups
        pool, dev, B, Cn, P = self.pool, self.device, idx.numel(), self.pool.channels, self.patch_size
        n2v = self.algorithm == NoiseAlgorithm.NOISE_TO_VOID
        box = n2v_ups._box_size() if n2v else 0
        if n2v and P % box:
            raise ValueError("device pool stream: Noise2Void needs a patch size that is a multiple of %d, got %d" % (box, P))
        cells = (P // box) ** 2 if n2v else 0
        f32 = dict(dtype=torch.float32, device=dev)
        inp = None
        if self._denoiser is not None and getattr(self._denoiser, "training", False):
            buf = self._denoiser.input_buffer(B, P, P, ncoords=(cells if n2v else 64))
            if buf is not None and tuple(buf.shape) == (B, Cn, P, P) and buf.device == dev:
                inp = buf
        if inp is None:
            inp = torch.empty((B, Cn, P, P), **f32)
        plain = torch.empty((B, Cn, P, P), **f32) if n2v else None
        par = torch.empty((B, Cn, 1, 1), **f32) if self.per_image else None
        coords = torch.empty((B, cells, 2), dtype=torch.int64, device=dev) if n2v else None
        origin = torch.empty((B, 3), dtype=torch.int32, device=dev) if self.keep_origin else None
        index = idx.to(torch.int32).to(dev, non_blocking=True)
        wide = pool.bits == 16
        a = L.PoolPatch16Args() if wide else L.PoolPatchArgs()
        if wide:
            a.white = pool.white
        a.pool, a.offsets, a.sizes, a.index = pool.pool.data_ptr(), pool.offsets.data_ptr(), pool.sizes.data_ptr(), index.data_ptr()
        a.params = pool.params.data_ptr() if self.per_image else None
        a.noisy32 = inp.data_ptr()
        a.ref32 = plain.data_ptr() if plain is not None else None
        a.coords = coords.data_ptr() if coords is not None else None
        a.param_out = par.data_ptr() if par is not None else None
        a.origin_out = origin.data_ptr() if origin is not None else None
        a.N, a.B, a.C, a.P = pool.n, B, Cn, P
        a.augment, a.n2v_box, a.n2v_radius = int(self.augment), box, 5 // 2
        a.seed, a.offset = self.seed, self._calls
        self._calls += 1
        rec = (L.OpRec * 1)()
        rec[0].type, rec[0].lane, rec[0].args = L.OP["pool_patch16" if wide else "pool_patch"], 0, C.cast(C.pointer(a), C.c_void_p)
        L.check(L.load().ssdn_run_ops(rec, 1, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        self.last_origin = origin
        return self._batch(idx, inp, plain, par, coords)

    def _prepare_torch(self, idx: torch.Tensor):
        from ssdn.utils import n2v_ups
        pool, g, B, Cn, P = self.pool, self.generator, idx.numel(), self.pool.channels, self.patch_size
        u8 = torch.empty((B, Cn, P, P), dtype=pool.pool.dtype, device=self.device)
        origin = torch.zeros((B, 3), dtype=torch.int32)
        for b, i in enumerate(idx.tolist()):
            rows, cols = (int(v) for v in pool.sizes_host[i])
            x0 = int(torch.randint(0, max(cols - P, 0) + 1, (1,), generator=g, device=self.device))
            y0 = int(torch.randint(0, max(rows - P, 0) + 1, (1,), generator=g, device=self.device))
            d = int(torch.randint(0, 8, (1,), generator=g, device=self.device)) if self.augment else 0
            origin[b] = torch.tensor([x0, y0, d], dtype=torch.int32)
            u8[b] = cut_patch(pool.image(i), P, x0, y0, d)
        self._calls += 1
        self.last_origin = origin if self.keep_origin else None
        if pool.bits == 16:                         # min(s, white) / white in fp32, as SSDN_OP_POOL_PATCH16
            plain = u8.to(torch.int32).clamp_(max=pool.white).to(torch.float32).div_(float(pool.white))
        else:
            plain = u8.to(torch.float32).div_(255.0)
        inp, coords = plain, None
        if self.algorithm == NoiseAlgorithm.NOISE_TO_VOID:
            inp, coords = n2v_ups.manipulate_batch(plain, 5, generator=g)
        par = None
        if self.per_image:
            par = pool.params[idx.to(self.device)].view(B, 1, 1, 1).expand(B, Cn, 1, 1).contiguous()
        return self._batch(idx, inp, plain if coords is not None else None, par, coords)
