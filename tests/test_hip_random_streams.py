"""GPU: the device random streams, element by element, against the exact host model tests/philox_ref.py: SSDN_OP_NOISE (csrc/elementwise.hip:
k_noise, k_noise_impulse), DevicePatchStream's (seed, offset) and the samples of SSDN_OP_HEAD_POSTERIOR (csrc/head_posterior.hip).  The
moment tests of test_hip_noise.py / test_hip_impulse.py / test_hip_posterior.py remain the tie to the reference package's distributions;
these pin the draw itself: which counter, which key, which word, which branch.

Every case keys the stream with a seed and an offset whose HIGH words carry information; test_philox_ref_cpu.py shows on the model alone
that no case has a fragile element (a float comparison one ulp could turn), so nothing is excluded here.  Tolerances: a normal draw is
compared within philox_ref.Z_TOL = 1e-3 standard normals (derived there from the kernel's only approximations, never from a measurement;
the measured deviation is printed: about 1e-6 is expected, above 1e-4 would be a finding), a ranged parameter within 2^-22 relative (the
kernel may fuse p_lo + (p_hi - p_lo) u), Poisson values within 1e-6 relative with the integer count exact, impulse values bit for bit."""
import math

import numpy as np
import pytest
import torch

import philox_ref as PR
from posterior_ops import posterior_op
from test_hip_noise import _run
from test_hip_posterior import _atol

pytestmark = pytest.mark.gpu
REL = 2.0 ** -22


def _launch(C, style, clip, lo, hi, seed=PR.SEED, offset=PR.OFFSET, n2v=False):
    """-> (u8, the kernel's outputs as numpy arrays, the model's)"""
    u8 = PR.case_image(C)
    o = _run(torch.from_numpy(u8), style, clip, lo, hi, seed=seed, offset=offset, ref=True, n2v=n2v)
    m = PR.noise_model(u8, style, clip, lo, hi, seed, offset, ref=True, n2v_box=8 if n2v else 0, n2v_radius=2)
    assert int(m["fragile"].sum()) == 0
    return u8, {k: (v.numpy() if v is not None else None) for k, v in o.items()}, m


def _check_deterministic_part(got, m, lo, hi, style):
    assert got["clean"].dtype == np.float32 and np.array_equal(got["clean"], m["clean"])
    for k in ("param", "param_ref"):
        if np.float32(lo) == np.float32(hi):
            assert np.array_equal(got[k], np.full(got[k].shape, np.float32(lo))), k                     # fixed: exact
        else:
            assert bool((np.abs(got[k].astype(np.float64) - m[k]) <= REL * np.abs(m[k])).all()), k
            assert float(got[k].min()) >= np.float32(lo) and float(got[k].max()) <= np.float32(hi)
            assert len(np.unique(got[k][:, 0])) == got[k].shape[0]
        if style == 2:
            assert bool((got[k] == got[k][:, :1]).all()), k          # ONE alpha per sample, written to all C entries


def _check_values(style, clip, got_v, want_v, clean, got_par, want_par, want_draw, what, blind=None):
    """one realisation against the model, per element, by the style's own tolerance.  `blind` [B,H,W]: the pixels a Noise2Void
    manipulation replaced: their VALUE is compared like any other, but it is not this pixel's clean value plus this pixel's draw"""
    g = got_v.astype(np.float64)
    own = np.ones(g.shape, dtype=bool) if blind is None else np.broadcast_to(~blind[:, None], g.shape)
    assert np.isfinite(g).all(), what
    if style == 0:
        bound = PR.Z_TOL * want_par[:, :, None, None] + REL
        err = np.abs(g - want_v)
        assert bool((err <= bound).all()), "%s: %d elements off, worst %.3e of %.3e" % (what, int((err > bound).sum()), float(err.max()), float(bound.max()))
        if not clip:
            dz = np.abs((g - clean) / want_par[:, :, None, None] - want_draw)[own]
            print("%s: max |z_kernel - z_model| = %.3e (max |z| %.2f)" % (what, float(dz.max()), float(np.abs(want_draw).max())))
    elif style == 1:
        assert bool((np.abs(g - want_v) <= 1e-6 * np.abs(want_v)).all()), what
        lam = got_par.astype(np.float64)[:, :, None, None]
        uncut = own if not clip else own & (g < 1.0) & (want_v < 1.0)                            # (the clip cuts from above only)
        k = (g - clean) * lam
        assert bool((np.abs(k - np.round(k)) < 1e-3)[uncut].all()), what
        assert np.array_equal(np.round(k)[uncut].astype(np.int64), want_draw[uncut]), what            # the integer count, exactly
        assert int(uncut.sum()) * 4 > uncut.size and int(want_draw.max()) >= 4
    else:
        assert np.array_equal(g, want_v), what                                                            # pure float32: bit for bit


def _check_case(C, style, clip, lo, hi, **kw):
    u8, got, m = _launch(C, style, clip, lo, hi, **kw)
    _check_deterministic_part(got, m, lo, hi, style)
    c64 = m["clean"].astype(np.float64)
    _check_values(style, clip, got["noisy"], m["noisy"], c64, got["param"], m["param"], m["draw"], "noisy", _blind(m))
    _check_values(style, clip, got["ref"], m["ref"], c64, got["param_ref"], m["param_ref"], m["draw_ref"], "ref")
    return u8, got, m


def _blind(m):
    """[B,H,W]: the pixels the model's Noise2Void manipulation replaced (None without one)"""
    if m["coords"] is None:
        return None
    blind = np.zeros(m["clean"][:, 0].shape, dtype=bool)
    for b in range(blind.shape[0]):
        blind[b, m["coords"][b, :, 1], m["coords"][b, :, 0]] = True
    return blind


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("style,clip,lo,hi", PR.GAUSS_CASES)
def test_gauss_draws_match_the_host_model(style, clip, lo, hi, C):
    _check_case(C, style, clip, lo, hi)


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("style,clip,lo,hi", PR.POISSON_CASES)
def test_poisson_counts_match_the_host_model(style, clip, lo, hi, C):
    _check_case(C, style, clip, lo, hi)


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("style,clip,lo,hi", PR.IMPULSE_CASES)
def test_impulse_hits_and_colours_match_the_host_model(style, clip, lo, hi, C):
    u8, got, m = _check_case(C, style, clip, lo, hi)
    for k, d in (("noisy", "draw"), ("ref", "draw_ref")):
        hit = m[d]
        assert np.array_equal(got[k][~hit], m["clean"][~hit])                          # untouched: exactly u8 / 255
        assert np.array_equal((got[k] != m["clean"]).any(1), hit[:, 0] & (m[k] != m["clean"]).any(1))      # the hit mask, per pixel
        share = float(hit.mean())
        assert abs(share - float(m["param" if k == "noisy" else "param_ref"].mean())) < 0.05


def _check_n2v(C, style, clip, lo, hi, seed=PR.SEED, offset=PR.OFFSET):
    u8, plain, _ = _launch(C, style, clip, lo, hi, seed=seed, offset=offset)
    u8, got, m = _check_case(C, style, clip, lo, hi, seed=seed, offset=offset, n2v=True)
    assert got["coords"].dtype == np.int64 and np.array_equal(got["coords"], m["coords"])
    blind = _blind(m)
    assert int(blind.sum()) == PR.B * 15
    # (_check_case compared every pixel of `noisy` with the model, whose blind pixels hold the value of THE drawn (rx, ry))
    assert bool((m["src"] != m["coords"]).any(-1).all())
    keep = np.broadcast_to(~blind[:, None], got["noisy"].shape)
    assert np.array_equal(got["noisy"][keep], plain["noisy"][keep])                    # every other pixel: the unmanipulated run, bit for bit
    for k in ("ref", "clean", "param", "param_ref"):
        assert np.array_equal(got[k], plain[k]), k
    return got, plain


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("style,clip,lo,hi", PR.N2V_CASES)
def test_noise2void_copies_the_drawn_neighbour(style, clip, lo, hi, C):
    got, plain = _check_n2v(C, style, clip, lo, hi)
    if style != 2:                                                                     # (an impulse copy may coincide with the old value)
        assert int((got["noisy"] != plain["noisy"]).any(1).sum()) >= PR.B * 15 - 3


@pytest.mark.parametrize("seed,offset", [(PR.SEED, PR.OFFSET_HI), (PR.SEED_HI, PR.OFFSET)])
@pytest.mark.parametrize("style,clip,lo,hi", PR.N2V_CASES)
def test_high_words_of_seed_and_offset_reach_the_counter_and_the_key(style, clip, lo, hi, seed, offset):
    """a seed / an offset that differs from the other tests' in the high word only: its own model, and another stream"""
    got, _ = _check_n2v(3, style, clip, lo, hi, seed=seed, offset=offset)
    base = _launch(3, style, clip, lo, hi, n2v=True)[1]
    assert not np.array_equal(got["noisy"], base["noisy"]) and not np.array_equal(got["ref"], base["ref"])
    assert not np.array_equal(got["coords"], base["coords"]) and (lo == hi or not np.array_equal(got["param"], base["param"]))


@pytest.mark.parametrize("name,algo,case,n2v", PR.STREAM_CASES)
def test_device_patch_stream_passes_its_seed_plus_rank_and_call_number(name, algo, case, n2v):
    """the n-th prepare of DevicePatchStream(seed=s, rank=r) is the op at seed s + r, offset n"""
    from ssdn.datasets import DevicePatchStream, NoisyDataset
    from ssdn.params import NoiseAlgorithm
    MD = NoisyDataset.Metadata
    style, clip, lo, hi = case
    nd = NoisyDataset(None, name, getattr(NoiseAlgorithm, algo), pad_uniform=False, pad_multiple=8, square=False, training_mode=True)
    u8 = PR.case_image(3)
    t, idx = torch.from_numpy(u8), torch.arange(PR.B)
    s = DevicePatchStream(None, nd, "cuda:0", seed=PR.STREAM_SEED, rank=PR.STREAM_RANK)
    for n in range(PR.STREAM_CALLS):
        inp, ref, md = s.prepare(t.pin_memory(), idx)
        m = PR.noise_model(u8, style, clip, lo, hi, PR.STREAM_SEED + PR.STREAM_RANK, n, ref=True, n2v_box=8 if n2v else 0, n2v_radius=2)
        assert int(m["fragile"].sum()) == 0
        c64 = m["clean"].astype(np.float64)
        assert np.array_equal(md[MD.CLEAN].cpu().numpy(), m["clean"])
        par = md[MD.INPUT_NOISE_VALUES].cpu().numpy().reshape(PR.B, -1)
        if lo == hi:
            assert np.array_equal(par, np.full(par.shape, np.float32(lo)))
            par = par_ref = np.full((PR.B, 3), np.float32(lo))
        else:
            assert par.shape == (PR.B, 3) and bool((np.abs(par - m["param"]) <= REL * m["param"]).all())
            par_ref = m["param_ref"].astype(np.float32)
        _check_values(style, clip, inp.cpu().numpy(), m["noisy"], c64, par, m["param"], m["draw"], "call %d input" % n, _blind(m))
        _check_values(style, clip, ref.cpu().numpy(), m["ref"], c64, par_ref, m["param_ref"], m["draw_ref"], "call %d reference" % n)
        if n2v:
            assert np.array_equal(md[MD.MASK_COORDS].cpu().numpy(), m["coords"])
    assert s.state_dict() == {"seed": PR.STREAM_SEED, "calls": PR.STREAM_CALLS}


@pytest.mark.parametrize("style,C,diag", PR.POSTERIOR_CASES)
def test_posterior_samples_match_the_host_model(style, C, diag):
    """B 2, 5x7, S 8, mode known: sample s of pixel b HW + p from streams 0x80000000 + 2 s (+ 1), through the mirror's float64 centre and
    factor.  Gaussian kinds: |x - model| <= sqrt(3) Z_TOL sqrt(cov_cc) (row c of L has norm sqrt(cov_cc), |dz| <= sqrt(3) Z_TOL) plus
    the tolerance test_hip_posterior.py grants the op's outputs against the mirror (rtol 2e-5, atol 1e-6 of the largest value, widened to
    at most 4x the fp32 mirror's own error).  Impulse: the keep decision wherever |u - w| exceeds 4x the fp32 mirror's own error in w
    (floor 1e-6; at most 1 % of the pairs may lie inside), kept samples are y bit for bit, the others within Z_TOL (|U| row sum) of
    mu_x + U z."""
    (no, y, npar, est), m, fig, model = PR.posterior_case(style, C, diag)
    S = PR.POSTERIOR_S
    runs = [posterior_op(no, y, npar, style, "known", est, diag=diag, nchunks=k, n_samples=S, seed=PR.SEED, offset=PR.OFFSET,
                         want=("samples",))["samples"].cpu() for k in (1, 2)]
    assert torch.isfinite(runs[0]).all() and torch.equal(runs[0], runs[1])
    x = runs[0].double().numpy()
    assert x.shape == model["samples"].shape
    if style != "impulse":
        cov = m["cov"].numpy()
        dg = np.maximum(cov[:, [0, 3, 5]] if C == 3 else cov, 0.0)
        tol_mean = 2e-5 * np.abs(model["samples"]) + _atol(1e-6 * float(m["mean"].abs().max()), fig["mean"])
        bound = math.sqrt(3) * PR.Z_TOL * np.sqrt(dg)[None] + tol_mean
        err = np.abs(x - model["samples"])
        print("%s C %d diag %d: worst |x - model| / bound = %.3f" % (style, C, diag, float((err / bound).max())))
        assert bool((err <= bound).all()), "%d samples off" % int((err > bound).sum())
        return
    w, y64 = m["w"].numpy(), y.double().numpy()
    band = max(1e-6, 4 * fig["w"])
    near = np.abs(model["u"].astype(np.float64) - w[None]) <= band
    print("impulse C %d: band %.2e, %d of %d (sample, pixel) pairs inside" % (C, band, int(near.sum()), near.size))
    assert int(near.sum()) * 100 <= near.size
    keep_model = model["u"].astype(np.float64) < w[None]
    keep_got = (x == y64[None]).all(2)                                                 # exactly the noisy pixel, in every channel
    assert np.array_equal(keep_got[~near], keep_model[~near])
    A = np.abs(no[:, C:].double().numpy())
    rows = np.stack([A[:, 0] + A[:, 1] + A[:, 2], A[:, 3] + A[:, 4], A[:, 5]] if C == 3 else [A[:, 0]], 1)
    err = np.abs(x - model["drawn"])
    ok = (err <= PR.Z_TOL * rows[None]).all(2)
    assert bool(ok[~keep_got].all()), "%d prior samples off" % int((~ok[~keep_got]).sum())
    assert 0 < int(keep_got.sum()) < keep_got.size
