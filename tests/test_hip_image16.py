"""GPU: the five 16-bit ops -- SSDN_OP_IMAGE_IN16 / IMAGE_OUT16 (csrc/image_io.hip), TILE_IN16 / TILE_OUT16 (csrc/tile_io.hip),
POOL_PATCH16 (csrc/patch_pool.hip) -- against the numpy model of tests/image16_ref.py bit for bit, against their byte siblings at
white = 255, their guards; `Denoiser.denoise` on uint16 images against the host route sample for sample, whole and tiled; training from a
16-bit pool; and `ssdn denoise` on a folder of both depths.

Nothing here has a tolerance: every op is an exact function of its inputs, and `denoise` runs the same plan on the same input bits as
the host route."""
import ctypes as C
import glob
import io
import os
import shutil

import numpy as np
import pytest
import torch

import image16_ref as R
import image_io_ref as IO
import patch_pool_ref as PP
import tile_ref as TR
from head_ops import DEV, P, run_one

pytestmark = pytest.mark.gpu
F32 = np.float32
OUT_GUARD = 64                  # elements in front of and behind every output of the pool op
BOX = 8                         # ssdn.utils.n2v_ups._box_size()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16)).to(DEV)


# ---- 1. IMAGE_IN16 / IMAGE_OUT16 against the model ----------------------------------------------------------------------------------------------
def image_in16_op(buf, count, offs, ext, Cn, H, W, white):
    """one SSDN_OP_IMAGE_IN16 launch on device copies -> dst [B,C,H,W] on the host; dst is NaN before the launch"""
    from ssdn.hip import lib as L
    B = len(offs)
    src = _dev16(buf)
    od = torch.tensor(offs, dtype=torch.int64, device=DEV)
    ed = torch.tensor(ext, dtype=torch.int32, device=DEV).contiguous()
    dst = torch.full((B, Cn, H, W), float("nan"), dtype=torch.float32, device=DEV)
    run_one("image_in16", L.ImageIn16Args(P(src), count, P(od), P(ed), B, Cn, H, W, white, P(dst)))
    return dst.cpu().numpy()


def image_out16_op(x, ext, offs, dst0, count, white, repeat=1):
    """`repeat` SSDN_OP_IMAGE_OUT16 launches on device copies -> the sample buffer on the host; it is dst0 before the first launch"""
    from ssdn.hip import lib as L
    B, Cn, H, W = x.shape
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    od = torch.tensor(offs, dtype=torch.int64, device=DEV)
    ed = torch.tensor(ext, dtype=torch.int32, device=DEV).contiguous()
    dst = _dev16(dst0.copy())
    for _ in range(repeat):
        run_one("image_out16", L.ImageOut16Args(P(xd), P(ed), P(od), P(dst), count, B, Cn, H, W, white))
    return dst.cpu().numpy()


def _planes(shape, seed, white):
    """an fp32 batch for IMAGE_OUT16: values around [0, 1] and beyond, k / white and its neighbours, .5 ties, and the special values"""
    g = np.random.default_rng(seed)
    x = g.uniform(-0.2, 1.2, shape).astype(F32)
    flat = x.reshape(-1)
    k = (g.integers(0, white + 1, size=300).astype(F32) / F32(white)).astype(F32)
    ties = ((g.integers(0, white, size=50).astype(np.float64) + 0.5) / white).astype(F32)
    special = np.concatenate([k, np.nextafter(k, F32(2)), np.nextafter(k, F32(-1)), ties,
                              np.array([-0.0, np.nan, np.inf, -np.inf, 1.0, -1e-30, 3e38], dtype=F32)])
    flat[g.choice(flat.size, special.size, replace=False)] = special
    return x


@pytest.mark.parametrize("white", R.WHITES)
@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("H,W", IO.PADDED)
def test_image_ops_against_the_numpy_model_bit_for_bit(H, W, Cn, white):
    """six images of EXTENTS in one packed buffer with 16 guard samples of 0xABCD between them; at white = 4095 an eighth of the samples
    lies above white.  Inside 32 x 96 three of the extents exceed the tensor: both sides clamp them to it"""
    ext = IO.EXTENTS
    images = R.make_images16(ext, Cn, 10 * H + Cn, white)
    assert white == 65535 or any((im > white).any() for im in images)
    buf, offs = R.pack_samples(images)
    got = image_in16_op(buf, buf.size, offs, ext, Cn, H, W, white)
    assert not np.isnan(got).any()                                   # every element was written
    want = R.image_in16_ref(buf, buf.size, offs, ext, Cn, H, W, white)
    assert np.array_equal(_bits(got), _bits(want)) and got.max() <= 1.0 and (white == 65535 or (got == 1.0).any())
    assert np.array_equal(_bits(image_in16_op(buf, buf.size, offs, ext, Cn, H, W, white)), _bits(got))
    # out: into a buffer of guard samples with a tail behind the last image
    x = _planes((len(ext), Cn, H, W), H + Cn, white)
    dst0 = np.full(buf.size + 64, R.GUARD_SAMPLE, dtype=np.uint16)
    out = image_out16_op(x, ext, offs, dst0, dst0.size, white)
    assert np.array_equal(out, R.image_out16_ref(x, ext, offs, dst0.copy(), dst0.size, white))
    mask = np.ones(dst0.size, dtype=bool)
    for b, (e1, e2) in enumerate(ext):
        mask[offs[b]:offs[b] + min(e1, H) * min(e2, W) * Cn] = False
    assert (out[mask] == R.GUARD_SAMPLE).all() and mask[-64:].all()
    assert np.array_equal(image_out16_op(x, ext, offs, dst0, dst0.size, white, repeat=2), out)


@pytest.mark.parametrize("white", R.WHITES)
@pytest.mark.parametrize("Cn", [1, 3])
def test_image_round_trip_on_the_device(Cn, white):
    ext = IO.fits(IO.EXTENTS, 64, 64)
    g = np.random.default_rng(3)
    images = [g.integers(0, white + 1, size=(e2, e1, Cn)).astype(np.uint16) for e1, e2 in ext]          # samples <= white
    buf, offs = R.pack_samples(images)
    x = image_in16_op(buf, buf.size, offs, ext, Cn, 64, 64, white)
    out = image_out16_op(x, ext, offs, np.full(buf.size, R.GUARD_SAMPLE, dtype=np.uint16), buf.size, white)
    assert np.array_equal(out, buf)


def test_inconsistent_tables_are_clamped_and_guarded():
    """The construction of the byte ops' test: the buffers are what the arguments say, only the tables are wrong -- extents beyond the
    tensor or negative, offsets that run past the count, start behind it or are negative, and a count below the buffer's size.  Reads
    outside give 0, writes outside are dropped, and the launch ends clean (the synchronize inside run_one raises otherwise)."""
    Cn, H, W, white = 3, 32, 64, 4095
    im = R.make_images16([(20, 30)], Cn, 5, white)[0]
    buf, offs = R.pack_samples([im] * 6)
    n = buf.size - 100                                               # the count the ops are told: the last image straddles it
    ext = [(20, 30), (999, 999), (-3, 30), (20, 30), (20, 30), (20, 30)]
    offs = [offs[0], offs[1], offs[2], n + 4096, -8, offs[5]]
    got = image_in16_op(buf, n, offs, ext, Cn, H, W, white)
    want = R.image_in16_ref(buf, n, offs, ext, Cn, H, W, white)
    assert np.array_equal(_bits(got), _bits(want))
    assert (got[2] == 0).all() and (got[3] == 0).all() and (got[4] == 0).all() and (got[5] == 0).any() and (got[5] != 0).any()
    x = _planes((6, Cn, H, W), 9, white)
    dst0 = np.full(buf.size, R.GUARD_SAMPLE, dtype=np.uint16)
    out = image_out16_op(x, ext, offs, dst0, n, white)
    assert np.array_equal(out, R.image_out16_ref(x, ext, offs, dst0.copy(), n, white))
    mask = np.ones(buf.size, dtype=bool)
    for b in (0, 1, 5):
        mask[offs[b]:min(offs[b] + min(ext[b][0], H) * min(ext[b][1], W) * Cn, n)] = False
    assert (out[mask] == R.GUARD_SAMPLE).all() and mask[n:].all() and mask[:16].all() and not mask[n - 1]
    torch.cuda.synchronize()


# ---- 2. TILE_IN16 / TILE_OUT16 against the model ----------------------------------------------------------------------------------------------
TILE_SIZES = [(70, 100), (33, 129), (65, 64), (1, 1)]               # (h, w)


def tile_in16_op(img, T, O, k0, B, white):
    from ssdn.hip import engine as E
    h, w, Cn = img.shape
    dst = torch.full((B, Cn, T, T), float("nan"), dtype=torch.float32, device=DEV)
    E.tile_in(_dev16(img.reshape(-1)), w, h, T, O, k0, dst, white=white)
    torch.cuda.synchronize()
    return dst.cpu().numpy()


def tile_out16_op(store, w, h, T, O, white, repeat=1):
    """`repeat` SSDN_OP_TILE_OUT16 launches into the middle of a buffer of guard samples -> (the image, the guards before and after it)"""
    from ssdn.hip import engine as E
    Cn, n = store.shape[1], w * h * store.shape[1]
    buf = _dev16(np.full(R.GUARD + n + R.GUARD, R.GUARD_SAMPLE, dtype=np.uint16))
    sd = torch.from_numpy(np.ascontiguousarray(store)).to(DEV)
    for _ in range(repeat):
        E.tile_out(sd, w, h, T, O, 0, buf[R.GUARD:R.GUARD + n], white=white)
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    return out[R.GUARD:R.GUARD + n].reshape(h, w, Cn), out[:R.GUARD], out[R.GUARD + n:]


def _agreeing_store(field, T, O):
    """field: float32 [h, w, C] -> the store whose tiles all hold the field (reflected beyond the image): they agree on every overlap"""
    h, w, Cn = field.shape
    Kx, Ky, S = TR.count(w, T, O), TR.count(h, T, O), T - O
    store = np.zeros((Kx * Ky, Cn, T, T), dtype=F32)
    for k in range(Kx * Ky):
        ky, kx = divmod(k, Kx)
        xs, ys = TR.reflect(kx * S + np.arange(T), w), TR.reflect(ky * S + np.arange(T), h)
        store[k] = field[ys[None, :], xs[:, None], :].transpose(2, 0, 1)
    return store


@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("T,O", TR.GPU_GRIDS)
def test_tile_ops_against_the_numpy_model_bit_for_bit(T, O, Cn):
    for (h, w), white in zip(TILE_SIZES, (65535, 4095, 4095, 65535)):
        img = R.make_images16([(w, h)], Cn, h + 3 * w + T, white)[0]
        want = R.tile_in16_ref(img, T, O, white)
        n = want.shape[0]
        # TILE_IN16: the whole grid in two calls (one where the grid is one tile)
        first = max(1, n // 2)
        for k0, B in ((0, first), (first, n - first)):
            if B < 1:
                continue
            got = tile_in16_op(img, T, O, k0, B, white)
            assert not np.isnan(got).any()                               # every element was written
            assert np.array_equal(_bits(got), _bits(want[k0:k0 + B])), (h, w, k0, B)
        # TILE_OUT16: a store of everything the blend and q16 must survive, NaN among it (NaN propagates, q16(NaN) = 0)
        store = R.make_store16(n, Cn, T, h + w + Cn, white)
        assert np.isnan(store).any() or n * Cn * T * T < 4000
        ref = R.tile_out16_ref(store, w, h, T, O, white)
        got, before, after = tile_out16_op(store, w, h, T, O, white)
        assert (before == R.GUARD_SAMPLE).all() and (after == R.GUARD_SAMPLE).all()        # nothing outside w h C samples is written
        assert got.dtype == np.uint16 and np.array_equal(got, ref), (h, w)
        blend = TR.blend_ref(store, w, h, T, O)
        assert (got.transpose(2, 0, 1)[np.isnan(blend)] == 0).all()
        again, _, _ = tile_out16_op(store, w, h, T, O, white, repeat=2)
        assert np.array_equal(again, got)
        # tiles that agree on their overlaps blend to exactly q16 of what they agree on
        field = np.random.default_rng(h + w).uniform(-0.2, 1.2, (h, w, Cn)).astype(F32)
        got, _, _ = tile_out16_op(_agreeing_store(field, T, O), w, h, T, O, white)
        assert np.array_equal(got, R.q16(field, white))
        # ... so the round trip on the device gives the samples back where they do not exceed white
        back, _, _ = tile_out16_op(want, w, h, T, O, white)
        assert np.array_equal(back, np.minimum(img, white))


# ---- 3. POOL_PATCH16 against the model ---------------------------------------------------------------------------------------------------------
class _Out:
    """an output between guards: poisoned (NaN; integers: a sentinel) before the launch"""

    def __init__(self, shape, dtype):
        self.n, self.shape = int(np.prod(shape)), shape
        self.poison = float("nan") if dtype.is_floating_point else -0x5A5A5A5A
        self.guard = 12345.0 if dtype.is_floating_point else 0x77777777
        self.buf = torch.full((self.n + 2 * OUT_GUARD,), self.guard, dtype=dtype, device=DEV)
        self.buf[OUT_GUARD:OUT_GUARD + self.n] = self.poison

    @property
    def ptr(self):
        return self.buf.data_ptr() + OUT_GUARD * self.buf.element_size()

    def read(self):
        h = self.buf.cpu().numpy()
        assert (h[:OUT_GUARD] == self.guard).all() and (h[OUT_GUARD + self.n:] == self.guard).all(), "guard overwritten"
        v = h[OUT_GUARD:OUT_GUARD + self.n].reshape(self.shape)
        assert not (np.isnan(v).any() if v.dtype.kind == "f" else (v == self.poison).any()), "an element was not written"
        return v


def _device_pool(images, params=None, wide=True):
    hp, off, sizes = R.pack16(images) if wide else PP.pack(images)
    return dict(pool=torch.from_numpy(hp).to(DEV), offsets=torch.from_numpy(off).to(DEV), sizes=torch.from_numpy(sizes).to(DEV).contiguous(),
                N=len(images), params=torch.tensor(params, dtype=torch.float32, device=DEV) if params is not None else None)


def pool_patch_op(dp, index, Cn, Pn, augment, seed, offset, n2v_box=0, white=None):
    """one SSDN_OP_POOL_PATCH16 launch (white None: the byte op) with every output between guards"""
    from ssdn.hip import lib as L
    B = len(index)
    idx = torch.tensor(index, dtype=torch.int32, device=DEV)
    cells = (Pn // n2v_box) ** 2 if n2v_box else 0
    noisy, ref = _Out((B, Cn, Pn, Pn), torch.float32), _Out((B, Cn, Pn, Pn), torch.float32)
    coords = _Out((B, cells, 2), torch.int64) if n2v_box else None
    par, org = _Out((B, Cn), torch.float32), _Out((B, 3), torch.int32)
    head = [P(dp["pool"]), P(dp["offsets"]), P(dp["sizes"]), P(dp["params"]), P(idx), noisy.ptr, ref.ptr, coords.ptr if coords else None,
            par.ptr if dp["params"] is not None else None, org.ptr, dp["N"], B, Cn, Pn, int(augment), n2v_box, 2]
    if white is None:
        run_one("pool_patch", L.PoolPatchArgs(*head, seed, offset))
    else:
        run_one("pool_patch16", L.PoolPatch16Args(*head, white, seed, offset))
    return dict(noisy=noisy.read(), ref=ref.read(), coords=coords.read() if coords else None,
                param=par.read() if dp["params"] is not None else None, origin=org.read())


def _pool_images16(Cn, white):
    rs = np.random.RandomState(177 + Cn)
    images = [rs.randint(0, white + 1, (Cn, r, c)).astype(np.uint16) for r, c in PP.SIZES]
    if white < 65535:
        for im in images:
            over = rs.randint(0, 8, im.shape) == 0
            im[over] = rs.randint(white + 1, 65536, int(over.sum()))
    return images


@pytest.mark.parametrize("white", R.WHITES)
@pytest.mark.parametrize("n2v_box", [0, BOX])
@pytest.mark.parametrize("augment", [False, True])
@pytest.mark.parametrize("Pn", [8, 32])
@pytest.mark.parametrize("Cn", [1, 3])
def test_pool_op_against_the_numpy_model_bit_for_bit(Cn, Pn, augment, n2v_box, white):
    images = _pool_images16(Cn, white)
    params = [0.01 * (i + 1) + 1 / 3 for i in range(len(images))]
    dp = _device_pool(images, params)
    assert any(int(o) % 2 for o in dp["offsets"].cpu())                  # odd sample offsets: nothing is aligned beyond a sample
    seen = set()
    for index, offset in zip(PP.INDEXES, (PP.OFFSETS[0], PP.OFFSETS[1], PP.OFFSETS[0])):
        got = pool_patch_op(dp, index, Cn, Pn, augment, PP.SEED, offset, n2v_box, white)
        m = R.pool_patch16_model(images, index, Pn, augment, PP.SEED, offset, white, params=params, n2v_box=n2v_box)
        assert np.array_equal(got["origin"], m["origin"])
        assert got["noisy"].dtype == np.float32 and np.array_equal(_bits(got["noisy"]), _bits(m["noisy"]))
        assert np.array_equal(_bits(got["ref"]), _bits(m["ref"])) and got["ref"].max() <= 1.0
        assert np.array_equal(got["param"], m["param"])
        if n2v_box:
            assert np.array_equal(got["coords"], m["coords"]) and (m["noisy"] != m["ref"]).any()
        else:
            assert np.array_equal(got["noisy"], got["ref"])
        seen |= set(index)
    assert seen == set(range(len(images)))


def test_pool_launch_refusals_launch_nothing():
    from ssdn.hip import lib as L
    images = _pool_images16(1, 65535)
    dp = _device_pool(images, [1.0] * 7)
    idx = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    out = _Out((2, 1, 8, 8), torch.float32)
    co = _Out((2, 1, 2), torch.int64)

    def args(**kw):
        a = L.PoolPatch16Args(P(dp["pool"]), P(dp["offsets"]), P(dp["sizes"]), P(dp["params"]), P(idx), out.ptr, None, None, None, None,
                              7, 2, 1, 8, 0, 0, 2, 65535, 1, 0)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(text, **kw):
        a = args(**kw)
        rec = (L.OpRec * 1)()
        rec[0].type, rec[0].lane, rec[0].args = L.OP["pool_patch16"], 0, C.cast(C.pointer(a), C.c_void_p)
        rc = L.load().ssdn_run_ops(rec, 1, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        msg = L.load().ssdn_last_error().decode()
        assert rc != 0 and "pool_patch16: " in msg and text in msg, (rc, msg)
    for name in ("pool", "offsets", "sizes", "index", "noisy32"):
        refused("are required", **{name: None})
    for name in ("N", "B", "C", "P"):
        refused("empty shape", **{name: 0})
    for white in (0, -1, 65536):
        refused("white must lie in [1, 65535]", white=white)
    refused("32-bit indexing", B=1 << 15, P=256)
    refused("params table", params=None, param_out=out.ptr)
    refused("coords output", n2v_box=8)
    refused("multiple of n2v_box", n2v_box=3, coords=co.ptr)
    refused("n2v_radius must be >= 1", n2v_box=8, coords=co.ptr, n2v_radius=0)
    refused("larger than 1 pixel", n2v_box=1, coords=co.ptr, P=1)
    refused("at most P", n2v_box=8, coords=co.ptr, n2v_radius=9)
    torch.cuda.synchronize()
    assert np.isnan(out.buf.cpu().numpy()[OUT_GUARD:OUT_GUARD + out.n]).all()      # nothing was launched
    run_one("pool_patch16", args())                                                 # ... and the unmodified arguments are accepted
    out.read()


# ---- 4. the three "in" ops at white = 255 against their byte siblings, launched side by side ------------------------------------------------------
@pytest.mark.parametrize("Cn", [1, 3])
def test_in_ops_at_white_255_equal_the_byte_ops(Cn):
    from ssdn.hip import engine as E
    from ssdn.hip import lib as L
    # IMAGE_IN16 / IMAGE_IN
    H, W = 64, 64
    ext = IO.fits(IO.EXTENTS, H, W)
    images = IO.make_images(ext, Cn, seed=40 + Cn)
    buf, offs = IO.pack(images)
    od = torch.tensor(offs, dtype=torch.int64, device=DEV)
    ed = torch.tensor(ext, dtype=torch.int32, device=DEV).contiguous()
    src8, dst8 = torch.from_numpy(buf).to(DEV), torch.full((len(ext), Cn, H, W), float("nan"), dtype=torch.float32, device=DEV)
    run_one("image_in", L.ImageInArgs(P(src8), buf.size, P(od), P(ed), len(ext), Cn, H, W, P(dst8)))
    got = image_in16_op(R.widen(buf), buf.size, offs, ext, Cn, H, W, 255)
    assert np.array_equal(_bits(got), _bits(dst8.cpu().numpy()))
    # TILE_IN16 / TILE_IN
    img = TR.make_image(70, 100, Cn, seed=Cn)
    n = TR.count(100, 64, 32) * TR.count(70, 64, 32)
    t8 = torch.full((n, Cn, 64, 64), float("nan"), dtype=torch.float32, device=DEV)
    E.tile_in(torch.from_numpy(img.reshape(-1)).to(DEV), 100, 70, 64, 32, 0, t8)
    assert np.array_equal(_bits(tile_in16_op(R.widen(img), 64, 32, 0, n, 255)), _bits(t8.cpu().numpy()))
    # POOL_PATCH16 / POOL_PATCH: values, and the draws
    imgs = PP.case_images(Cn)
    d8, d16 = _device_pool(imgs, [0.5] * 7, wide=False), _device_pool([R.widen(im) for im in imgs], [0.5] * 7)
    for box in (0, BOX):
        a = pool_patch_op(d8, PP.INDEXES[2], Cn, 32, True, PP.SEED, PP.OFFSETS[0], box)
        b = pool_patch_op(d16, PP.INDEXES[2], Cn, 32, True, PP.SEED, PP.OFFSETS[0], box, white=255)
        assert np.array_equal(a["origin"], b["origin"]) and (box == 0 or np.array_equal(a["coords"], b["coords"]))
        for k in ("noisy", "ref", "param"):
            assert np.array_equal(_bits(a[k]), _bits(b[k])), k


# ---- 5. Denoiser.denoise on uint16 against the host route ------------------------------------------------------------------------------------------
# (name, algorithm, style, noise value, channels, noise_param of the call, its value in the metadata)
MODELS = [("ssdn_gauss_known_mono", "ssdn", "gauss25", "known", 1, 25, 25 / 255),
          ("n2c_rgb", "n2c", "gauss25", None, 3, None, None)]
SIZES = [(24, 40), (64, 64), (50, 33)]                               # (h, w)
_DEN = {}


def _model(name):
    """the model `name` with random weights (the constructor's He-normal draw under a fixed seed), built once and shared"""
    if name not in _DEN:
        import ssdn
        from ssdn.denoiser import Denoiser
        from ssdn.params import ConfigValue, NoiseAlgorithm, NoiseValue
        _, alg, style, mode, ch, _, _ = next(m for m in MODELS if m[0] == name)
        cfg = ssdn.cfg.base()
        cfg[ConfigValue.ALGORITHM] = NoiseAlgorithm(alg)
        cfg[ConfigValue.NOISE_STYLE] = style
        cfg[ConfigValue.IMAGE_CHANNELS] = ch
        if mode is not None:
            cfg[ConfigValue.NOISE_VALUE] = NoiseValue(mode)
        torch.manual_seed(11)
        d = Denoiser(ssdn.cfg.infer(cfg, model_only=True), device="cuda:0")
        d.mark_dirty()
        _DEN[name] = d
    return _DEN[name]


def _images16(ch, white, seed=0, sizes=SIZES):
    return R.make_images16([(w, h) for h, w in sizes], ch, 100 + seed, white)


def _padded_shapes(images, blind, uniform, bucket=32):
    up = lambda n: (n + bucket - 1) // bucket * bucket      # noqa: E731
    big = (max(im.shape[1] for im in images), max(im.shape[0] for im in images))
    res = []
    for im in images:
        H, W = (up(n) for n in (big if uniform else (im.shape[1], im.shape[0])))
        res.append((max(H, W),) * 2 if blind else (H, W))
    return res


def _data(x, npv):
    from ssdn.datasets import NoisyDataset
    data = [x]
    if npv is not None:
        data += [torch.zeros(0), {NoisyDataset.Metadata.INPUT_NOISE_VALUES: torch.full((x.shape[0], 1, 1, 1), npv)}]
    return data


@pytest.mark.parametrize("white", R.WHITES)
@pytest.mark.parametrize("uniform", [False, True])
@pytest.mark.parametrize("name", [m[0] for m in MODELS])
def test_denoise_of_uint16_is_the_host_route_sample_for_sample(name, uniform, white):
    from ssdn.params import ConfigValue, PipelineOutput as PO
    _, alg, style, mode, ch, npar, npv = next(m for m in MODELS if m[0] == name)
    d = _model(name)
    is_ssdn = alg == "ssdn"
    images = _images16(ch, white)
    d.train()                                                        # whatever the module's mode
    res = d.denoise(images, noise_param=npar, batch_size=2, uniform=uniform, std=is_ssdn, white=None if white == 65535 else white)
    assert d.training and set(res) == ({"out", "noise_std", "std"} if is_ssdn else {"out"})
    shapes = _padded_shapes(images, d.cfg[ConfigValue.BLINDSPOT], uniform)
    groups = {}
    for k, s in enumerate(shapes):
        groups.setdefault(s, []).append(k)
    d.eval()
    for (H, W), members in groups.items():
        for lo in range(0, len(members), 2):
            idx = members[lo:lo + 2]
            batch = [images[k] for k in idx]
            # the padded fp32 input from the definition: the images packed back to back, ext = (w, h)
            buf, offs = R.pack_samples(batch)
            ext = [(im.shape[1], im.shape[0]) for im in batch]
            x = torch.from_numpy(R.image_in16_ref(buf, buf.size, offs, ext, ch, H, W, white)).to(DEV)
            with torch.no_grad():
                out = d.run_pipeline(_data(x, npv))
            den = out[PO.IMG_DENOISED].cpu().numpy()
            post = d.posterior(_data(x, npv))["std"].cpu() if is_ssdn else None
            for b, k in enumerate(idx):
                h, w = SIZES[k]
                got = res["out"][k]
                assert got.dtype == torch.uint16 and tuple(got.shape) == (h, w, ch) and got.device.type == "cpu"
                want = R.q16(den[b, :, :w, :h], white).transpose(2, 1, 0)
                assert np.array_equal(got.numpy(), want), (name, uniform, white, k)
                assert len(np.unique(want)) > 8 and want.max() <= white
                if is_ssdn:
                    assert torch.equal(res["std"][k], post[b, :, :w, :h].permute(0, 2, 1))


def test_tiled_denoise_of_uint16_is_the_host_composition():
    """a 70 x 100 image at tile = 64, overlap = 32, two tiles per batch: the model's tiles through the same plan, its blend and q16"""
    from ssdn.params import PipelineOutput as PO
    name, T, O, white = "ssdn_gauss_known_mono", 64, 32, 4095
    _, _, _, _, ch, npar, npv = MODELS[0]
    d = _model(name)
    img = _images16(ch, white, seed=3, sizes=[(70, 100)])[0]
    res = d.denoise([img[:, :, 0]], noise_param=npar, batch_size=2, std=True, tile=T, overlap=O, white=white)
    tiles = R.tile_in16_ref(img, T, O, white)
    n = tiles.shape[0]
    assert res["tiles"] == [n] and n == 6
    store, store_std = np.zeros_like(tiles), np.zeros_like(tiles)
    d.eval()
    for k0 in range(0, n, 2):
        data = _data(torch.from_numpy(tiles[k0:k0 + 2]).to(DEV), npv)
        with torch.no_grad():
            out = d.run_pipeline(data)
        store[k0:k0 + 2] = out[PO.IMG_DENOISED].cpu().numpy()
        store_std[k0:k0 + 2] = d.posterior(data)["std"].cpu().numpy()
    got = res["out"][0]
    assert got.dtype == torch.uint16 and tuple(got.shape) == (70, 100)               # [h, w] in, [h, w] out
    assert np.array_equal(got.numpy(), R.tile_out16_ref(store, 100, 70, T, O, white)[:, :, 0])
    assert np.array_equal(_bits(res["std"][0].numpy()), _bits(TR.tile_out_ref(store_std, 100, 70, T, O, 1)))


def test_a_call_of_both_depths_leaves_the_bytes_alone():
    d = _model("ssdn_gauss_known_mono")
    g = np.random.default_rng(8)
    b8 = [g.integers(0, 256, size=(h, w, 1), dtype=np.uint8) for h, w in SIZES]
    w16 = _images16(1, 65535, seed=5)
    for uniform in (False, True):
        alone = d.denoise(b8, noise_param=25, batch_size=2, uniform=uniform, std=True)
        only16 = d.denoise(w16, noise_param=25, batch_size=2, uniform=uniform, std=True)
        mixed = d.denoise([b8[0], w16[0], w16[1], b8[1], b8[2], w16[2]], noise_param=25, batch_size=2, uniform=uniform, std=True)
        for pos, (src, k) in enumerate(((alone, 0), (only16, 0), (only16, 1), (alone, 1), (alone, 2), (only16, 2))):
            assert mixed["out"][pos].dtype == src["out"][k].dtype and torch.equal(mixed["out"][pos], src["out"][k])
            assert torch.equal(mixed["std"][pos], src["std"][k]) and mixed["noise_std"][pos] == src["noise_std"][k]
    with pytest.raises(ValueError, match="estimator is defined on bytes"):
        d.denoise([b8[0], w16[0]], noise_param="auto")


# ---- 6. training from a 16-bit pool ----------------------------------------------------------------------------------------------------------------
def _folders(root):
    """four 40 x 40 grey pictures three times: as 8-bit PNGs, as 16-bit PNGs holding the same values, and scaled to the full 16-bit range"""
    from PIL import Image
    rs = np.random.RandomState(2)
    arrays = []
    for k in range(4):
        yy, xx = np.mgrid[0:40, 0:40]
        base = 0.5 + 0.3 * np.sin(xx / (5.0 + k)) * np.cos(yy / 7.0) + rs.randn(40, 40) * (25 / 255.0)
        arrays.append(np.uint8(np.clip(base, 0, 1) * 255))
    for name, conv in (("b8", lambda a: a), ("w255", lambda a: a.astype(np.uint16)), ("w65535", lambda a: a.astype(np.uint16) * 257)):
        os.makedirs(str(root / name))
        for k, a in enumerate(arrays):
            Image.fromarray(conv(a)).save(str(root / name / ("im%d.png" % k)))
    return arrays


def _train_cli(root, folder, runs, extra=()):
    from ssdn.__main__ import start_cli
    torch.manual_seed(20261021)          # weights, sampling order and the crop stream all derive from the host RNG
    return start_cli(["train", "start", "--noisy", "-a", "ssdn", "--noise_value", "known", "-n", "gauss25", "--mono", "-t", str(root / folder),
                      "-i", "6", "--train_batch_size", "2", "--patch_size", "32", "--print_interval", "2", "--checkpoint_interval", "2",
                      "--runs_dir", str(root / runs)] + list(extra))


def _tensors(o, pre=""):
    if torch.is_tensor(o):
        yield pre, o
    elif isinstance(o, dict):
        for k in o:
            yield from _tensors(o[k], pre + "/" + str(k))


@pytest.fixture(scope="module")
def runs16(tmp_path_factory):
    root = tmp_path_factory.mktemp("runs16")
    arrays = _folders(root)
    return root, arrays, _train_cli(root, "b8", "runs8"), _train_cli(root, "w255", "runs255", ["--white", "255"])


def test_a_16_bit_run_at_white_255_is_the_8_bit_run_bit_for_bit(runs16):
    from ssdn.datasets import DevicePoolStream
    from ssdn.params import StateValue
    from test_hip_trainer import _scalars
    _, _, t8, t16 = runs16
    assert isinstance(t16.trainloader, DevicePoolStream) and t16.trainloader.pool.bits == 16 and t16.trainloader.pool.white == 255
    assert t8.trainloader.pool.bits == 8 and t8.state[StateValue.ITERATION] == t16.state[StateValue.ITERATION] == 6
    a, b = _scalars(t8.run_dir_path)["train/loss"], _scalars(t16.run_dir_path)["train/loss"]
    assert [s for s, _ in a] == [2, 4, 6] and a == b and all(np.isfinite(v) for _, v in a)            # one line per step of batch 2
    fa = torch.load(glob.glob(os.path.join(t8.run_dir_path, "final-*.wt"))[0], map_location="cpu", weights_only=False)
    fb = torch.load(glob.glob(os.path.join(t16.run_dir_path, "final-*.wt"))[0], map_location="cpu", weights_only=False)
    ta, tb = dict(_tensors(fa)), dict(_tensors(fb))
    assert ta.keys() == tb.keys() and len(ta) > 10 and all(torch.equal(ta[k], tb[k]) for k in ta)
    last = os.path.join("training", "model_00000006.training")
    sd8 = torch.load(os.path.join(t8.run_dir_path, last), map_location="cpu", weights_only=False)
    sd16 = torch.load(os.path.join(t16.run_dir_path, last), map_location="cpu", weights_only=False)
    assert sd8["noisy"] == {"mode": "style", "augment": False, "pool_bytes": None} and sd16["noisy"] == dict(sd8["noisy"], white=255)


def test_step_losses_from_the_two_pools_are_equal_bit_for_bit(runs16):
    """the same three minibatches cut out of the 8-bit pool and out of the 16-bit pool at white = 255, through two equal models"""
    from ssdn.datasets import DevicePoolStream, ImagePool, UnlabelledImageFolderDataset
    from ssdn.params import NoiseAlgorithm, PipelineOutput as PO
    from test_hip_denoiser import make_denoiser
    root = runs16[0]
    torch.manual_seed(77)
    d1 = make_denoiser("ssdn", "gauss25", "known", 1)
    d2 = make_denoiser("ssdn", "gauss25", "known", 1)
    d2.load_state_dict(d1.state_dict())
    d2.mark_dirty()
    batches = [[0, 3], [2, 1], [3, 3]]
    losses = []
    for d, folder, white in ((d1, "b8", None), (d2, "w255", 255)):
        pool = ImagePool(UnlabelledImageFolderDataset(str(root / folder), channels=1), DEV, white=white)
        st = DevicePoolStream(pool, batches, NoiseAlgorithm.SELFSUPERVISED_DENOISING, "gauss25", 32, augment=True, seed=3).attach(d)
        d.train()
        losses.append([d.train_step(data, 1e-3)[PO.LOSS].detach().clone() for data in st])
    torch.cuda.synchronize()
    assert len(losses[0]) == 3 and all(torch.isfinite(x).all() and torch.equal(x, y) for x, y in zip(*losses))
    assert torch.equal(d1.flat, d2.flat)


def test_a_full_range_pool_trains_and_its_minibatch_is_the_model(runs16):
    from ssdn.datasets import DevicePoolStream, ImagePool, UnlabelledImageFolderDataset
    from ssdn.params import NoiseAlgorithm, PipelineOutput as PO
    from test_hip_denoiser import make_denoiser
    root, arrays = runs16[:2]
    pool = ImagePool(UnlabelledImageFolderDataset(str(root / "w65535"), channels=1), DEV)
    assert pool.bits == 16 and pool.white == 65535 and pool.pool.dtype == torch.uint16 and pool.nbytes == 2 * 4 * 40 * 40
    planar = [(a.astype(np.uint16) * 257).T[None] for a in arrays]                       # [1, rows = w, cols = h]
    assert all(np.array_equal(pool.image(i).cpu().numpy(), planar[i]) for i in range(4))
    torch.manual_seed(78)
    d = make_denoiser("ssdn", "gauss25", "known", 1)
    d.train()
    batches = [[1, 2], [0, 3], [2, 2]]
    st = DevicePoolStream(pool, batches, NoiseAlgorithm.SELFSUPERVISED_DENOISING, "gauss25", 32, augment=True, seed=4).attach(d)
    st.keep_origin = True
    for n, (idx, data) in enumerate(zip(batches, st)):
        if n == 0:
            want = np.stack([R.sample_in(PP.cut(planar[i], 32, *[int(v) for v in st.last_origin[b].cpu()]), 65535) for b, i in enumerate(idx)])
            assert np.array_equal(_bits(data[0].cpu().numpy()), _bits(want))
        assert torch.isfinite(d.train_step(data, 1e-3)[PO.LOSS]).all()
    torch.cuda.synchronize()
    assert data[0].data_ptr() == d.input_buffer(2, 32, 32).data_ptr()        # (once the engine exists) written straight into its input buffer
    with pytest.raises(ValueError, match="estimator is defined on bytes"):
        pool.estimate_params(d, "gauss")


def test_resume_restores_white(runs16):
    from ssdn.params import StateValue
    from ssdn.train import resume_run
    root, _, _, t16 = runs16
    run = t16.run_dir_path
    copy = str(root / "runs_resumed" / os.path.basename(run))
    shutil.copytree(run, copy)
    for p in glob.glob(os.path.join(copy, "final-*.wt")) + [os.path.join(copy, "training", "model_00000006.training")]:
        os.remove(p)
    r = resume_run(copy, iteration=4)
    assert r.noisy == "style" and r.white == 255 and r.state[StateValue.ITERATION] == 4
    r.train()
    assert r.state[StateValue.ITERATION] == 6 and r.trainloader.pool.bits == 16 and r.trainloader.pool.white == 255
    a = torch.load(glob.glob(os.path.join(run, "final-*.wt"))[0], map_location="cpu", weights_only=False)
    b = torch.load(glob.glob(os.path.join(copy, "final-*.wt"))[0], map_location="cpu", weights_only=False)
    ta, tb = dict(_tensors(a)), dict(_tensors(b))
    assert ta.keys() == tb.keys() and all(torch.equal(ta[k], tb[k]) for k in ta)


# ---- 7. the command, end to end -------------------------------------------------------------------------------------------------------------------
def test_cli_denoise_on_a_folder_of_both_depths(tmp_path):
    from PIL import Image
    from ssdn.__main__ import start_cli
    from ssdn.denoiser import Denoiser
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    a16 = _images16(1, 4095, seed=6, sizes=[(24, 40)])[0][:, :, 0]
    a8 = np.random.default_rng(21).integers(0, 256, size=(33, 50), dtype=np.uint8)
    Image.fromarray(a16).save(imgs / "a16.png")
    Image.fromarray(a8).save(imgs / "b8.png")
    d = _model("ssdn_gauss_known_mono")
    torch.save({k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in d.state_dict().items()}, tmp_path / "model.wt")
    out_dir = tmp_path / "out"
    start_cli(["denoise", "-m", str(tmp_path / "model.wt"), "-i", str(imgs), "-o", str(out_dir), "--noise_param", "25", "--white", "4095"])
    fresh = Denoiser.from_state_dict(torch.load(tmp_path / "model.wt", map_location="cpu", weights_only=False))
    want16 = fresh.denoise([a16], noise_param=25, white=4095)["out"][0]
    want8 = fresh.denoise([a8], noise_param=25)["out"][0]
    assert sorted(os.listdir(out_dir)) == ["a16.png", "b8.png", "denoise.csv"]
    with Image.open(out_dir / "a16.png") as im:
        assert im.mode == "I;16" and np.array_equal(np.asarray(im), want16.numpy()) and want16.dtype == torch.uint16
    # the 8-bit picture: the very file the command writes for it alone
    mem = io.BytesIO()
    Image.fromarray(want8.numpy()).save(mem, format="PNG")
    assert open(out_dir / "b8.png", "rb").read() == mem.getvalue()
    rows = open(out_dir / "denoise.csv").read().splitlines()
    assert rows[0] == "file,width,height,noise_std" and rows[1].startswith("a16.png,40,24,") and rows[2].startswith("b8.png,50,33,")
    with pytest.raises(ValueError, match="estimator is defined on bytes.*pass the noise parameter as a number"):
        start_cli(["denoise", "-m", str(tmp_path / "model.wt"), "-i", str(imgs), "-o", str(tmp_path / "out2"), "--noise_param", "auto"])
    assert not os.path.exists(tmp_path / "out2")
