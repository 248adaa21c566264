"""CPU: the host model of the library's random streams (tests/philox_ref.py) on its own: Philox4x32-10 against the published known-answer
vectors, the endpoints of u01, the Poisson inversion's thresholds, n2v_pick against brute force, and the conditions the GPU tests
(tests/test_hip_random_streams.py) rest on: no fragile element in any of their cases, at most 1 % of the impulse posterior's keep decisions
inside the band of the weight's own fp32 error."""
import math

import numpy as np
import pytest

import philox_ref as PR


# Random123's kat_vectors for philox4x32 with 10 rounds: (counter; key) -> output
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_philox_known_answer_vectors():
    for ctr, key, want in KAT:
        assert tuple(int(v) for v in PR.philox4x32_10(*ctr, *key)) == want
    # ... and vectorised: the three at once, each in its own lane
    got = PR.philox4x32_10(*[np.array([k[0][i] for k in KAT]) for i in range(4)], *[np.array([k[1][i] for k in KAT]) for i in range(2)])
    assert [tuple(int(w[n]) for w in got) for n in range(3)] == [k[2] for k in KAT]


def test_u01_endpoints_and_the_largest_normal():
    """u01 maps to (0, 1], not (0, 1): (2^24 - 0.5) / 2^24 rounds up to 1.0 in fp32.  The smallest value 2^-25 bounds every normal by
    sqrt(-2 ln 2^-25) = sqrt(50 ln 2); u = 1.0 gives ln 1 = 0, a normal of exactly 0"""
    assert PR.u01(0).dtype == np.float32
    assert float(PR.u01(0)) == 2.0 ** -25 and float(PR.u01(0xFF)) == 2.0 ** -25 and float(PR.u01(0x100)) == 2.0 ** -24 + 2.0 ** -25
    # in [0.5, 1) fp32 steps by 2^-24 and the added 2^-25 is a tie, rounded to even: the top word gives 1.0, the next ones 1 - 2^-23
    assert float(PR.u01(0xFFFFFFFF)) == 1.0 and float(PR.u01(0xFFFFFEFF)) == 1.0 - 2.0 ** -23 and float(PR.u01(0xFFFFFDFF)) == 1.0 - 2.0 ** -23
    words = np.array([0, 0x100, 0x7FFFFFFF, 0x80000000, 0xFFFFFEFF, 0xFFFFFFFF])
    assert bool((PR.u01(words) > 0).all()) and bool((PR.u01(words) <= 1).all())
    # the radius is largest at word 0, |cos| reaches 1 at both ends of u (up to the fp32 constant for 2 pi)
    bound = math.sqrt(50 * math.log(2))
    zmax = float(PR.normal(0, 0xFFFFFFFF))
    assert zmax == pytest.approx(bound, rel=1e-12) and zmax == pytest.approx(5.887, abs=5e-4)
    grid = np.arange(0, 1 << 32, 1 << 20)
    assert float(np.abs(PR.normal(0, grid)).max()) <= bound * (1 + 1e-14)
    assert float(np.abs(PR.normal(grid, grid[::-1])).max()) <= bound
    assert float(PR.normal(0xFFFFFFFF, 12345)) == 0.0
    z0, z1 = PR.normal2(0x12345678, 0x5ABCDEF0)
    assert float(z0) == float(PR.normal(0x12345678, 0x5ABCDEF0))
    r2 = -2.0 * math.log(float(PR.u01(0x12345678)))
    assert float(z0) ** 2 + float(z1) ** 2 == pytest.approx(r2, rel=1e-12) and float(z1) > 0      # u(b) = 0.354: cosine < 0 < sine
    assert float(z0) < 0


def test_poisson_thresholds_make_the_cap_unreachable():
    """The float32 cdf values increase and reach 1 - 2^-24 or more before k = 16 (T[10] is exactly 1.0), so `u > cdf` fails for every
    u01 below 1.0 and the loop never ends by its cap; T[9] = 1 - 2^-23 is the largest u01 below 1.0 itself, so such a u gives k <= 9.
    u01 == 1.0 (the top 256 words of 2^32): 1.0 > T[10] = 1.0 fails, k = 10, no cap either (P(k >= 10) is 1.1e-7, the words give 6.0e-8)."""
    t = PR.poisson_thresholds()
    assert t.dtype == np.float32 and len(t) == 17
    assert float(t[0]) == float(np.float32(0.36787944117))
    assert bool((np.diff(t.astype(np.float64)) >= 0).all())
    first = int(np.argmax(t >= np.float32(1.0 - 2.0 ** -24)))
    assert float(t[first]) >= 1.0 - 2.0 ** -24 and 0 < first < 16
    assert bool((np.diff(t[:first + 1].astype(np.float64)) > 0).all())          # strictly increasing until it saturates
    exact = np.cumsum([math.exp(-1) / math.factorial(k) for k in range(17)])
    assert float(np.abs(t.astype(np.float64) - exact).max()) < 2.0 ** -22
    big = np.float32(1.0 - 2.0 ** -23)                                           # the largest u01 below 1.0
    k, _ = PR.poisson1(np.array([2.0 ** -25, 0.36, 0.37, 0.735, 0.74, big], dtype=np.float32))
    assert k.tolist()[:5] == [0, 0, 1, 1, 2] and int(k[5]) <= first
    k1, _ = PR.poisson1(np.array([1.0], dtype=np.float32))
    assert float(t[first]) == 1.0 and int(k1[0]) == first == 10
    assert float(t[9]) == 1.0 - 2.0 ** -23 and int(k[5]) == 9
    # the loop, literally, agrees with the count of thresholds below u
    us = PR.u01(np.arange(0, 1 << 32, (1 << 32) // 4099))
    kk, _ = PR.poisson1(us)
    for u, want in zip(us.tolist() + [1.0], kk.tolist() + [int(k1[0])]):
        u, pk, n = np.float32(u), np.float32(0.36787944117), 0
        cdf = pk
        while u > cdf and n < 16:
            n += 1
            pk = np.float32(pk / np.float32(n))
            cdf = np.float32(cdf + pk)
        assert n == want


def _candidates(c, size, r=2):
    """the candidate set tests/test_hip_noise.py::_check_n2v_geometry enumerates"""
    return sorted({v % size for v in range(min(c - r, 0), min(c + r, size - 1)) if v != c})


def test_n2v_pick_against_brute_force():
    words = np.concatenate([np.array([0, 0xFF, 0x100, 0xFFFFFEFF, 0xFFFFFF00, 0xFFFFFFFF], dtype=np.uint64),
                            np.arange(4090, dtype=np.uint64) * np.uint64(1050011) + np.uint64(77)])
    assert len(words) == 4096 and int(words.max()) <= 0xFFFFFFFF
    u = PR.u01(words)
    for size in (8, 24, 40):
        for c in range(size):
            cand = _candidates(c, size)
            got = PR.n2v_pick(c, 2, size, u)
            assert set(got.tolist()) == set(cand), (c, size)                  # always a candidate, and every candidate is reached
            assert c not in got.tolist(), (c, size)
            # the literal function of the kernel, per word
            lo, hi = (c - 2 if c - 2 < 0 else 0), (c + 2 if c + 2 < size - 1 else size - 1)
            inside = c >= lo and c < hi
            span = max(hi - lo - (1 if inside else 0), 1)
            for n in (0, 1, 2, 3, 4, 5, 6, 2000, 4095):
                k = min(int(np.float32(u[n]) * np.float32(span)), span - 1)
                v = lo + k
                v = v + 1 if inside and v >= c else v
                v = v + size if v < 0 else v
                assert min(v, size - 1) == int(got[n])


def test_no_case_of_the_gpu_tests_has_a_fragile_element():
    """so the GPU tests compare EVERY element: nothing is excluded"""
    runs = PR.all_noise_runs()
    assert len(runs) == len(set(runs))
    for C, style, clip, lo, hi, seed, offset, n2v in runs:
        m = PR.noise_model(PR.case_image(C), style, clip, lo, hi, seed, offset, ref=True, n2v_box=8 if n2v else 0, n2v_radius=2)
        assert m["fragile"].shape == (PR.B, C, PR.H, PR.W) and int(m["fragile"].sum()) == 0, (C, style, clip, lo, hi, seed, offset, n2v)
    # the band is not empty by construction: a u01 next to a threshold, or next to a ranged alpha, is reported
    t = PR.poisson_thresholds()
    _, fr = PR.poisson1(np.array([t[1], t[1] + np.float32(2.0 ** -23), 0.5], dtype=np.float32))
    assert fr.tolist() == [True, True, False]


def test_the_model_of_a_small_case_by_hand():
    """one element of each style, recomputed from the words"""
    u8 = PR.case_image(3)
    sd, off = PR.SEED, PR.OFFSET
    b, c, y, x = 1, 2, 17, 33
    HW = PR.H * PR.W
    e = (b * 3 + c) * HW + y * PR.W + x
    w = PR.philox4x32_10(e, 0, 9, 3, 7, 5)
    g = PR.noise_model(u8, 0, False, 0.1, 0.1, sd, off)
    assert float(g["noisy"][b, c, y, x]) == pytest.approx(float(g["clean"][b, c, y, x]) + float(np.float32(0.1)) * float(PR.normal(w[0], w[1])), abs=1e-15)
    assert float(g["param"][b, c]) == float(np.float32(0.1)) and g["coords"] is None
    wr = PR.philox4x32_10(e, 1, 9, 3, 7, 5)
    p = PR.noise_model(u8, 1, False, 30.0, 30.0, sd, off)
    k = int(PR.poisson1(PR.u01(wr[0]))[0])
    assert int(p["draw_ref"][b, c, y, x]) == k and float(p["ref"][b, c, y, x]) == pytest.approx(float(p["clean"][b, c, y, x]) + k / 30.0, rel=1e-14)
    wi = PR.philox4x32_10(b * HW + y * PR.W + x, 0, 9, 3, 7, 5)
    i = PR.noise_model(u8, 2, False, 0.5, 0.5, sd, off)
    hit = float(PR.u01(wi[0])) < 0.5
    assert bool(i["draw"][b, c, y, x]) == hit
    assert float(i["noisy"][b, c, y, x]) == (float(PR.u01(wi[1 + c])) if hit else float(np.float32(u8[b, c, y, x]) / np.float32(255)))
    # Noise2Void: one coordinate per box in the reference's order, the source is a candidate and the value is the source's
    n = PR.noise_model(u8, 0, False, 0.1, 0.1, sd, off, n2v_box=8)
    ny = PR.H // 8
    for bb in range(PR.B):
        assert [(cx // 8) * ny + cy // 8 for cx, cy in n["coords"][bb].tolist()] == list(range(15))
        for (cx, cy), (rx, ry) in zip(n["coords"][bb].tolist(), n["src"][bb].tolist()):
            assert rx in _candidates(cx, PR.W) and ry in _candidates(cy, PR.H)
            assert np.array_equal(n["noisy"][bb, :, cy, cx], g["noisy"][bb, :, ry, rx])
    changed = (n["noisy"] != g["noisy"]).any(1)
    assert int(changed.sum()) <= 30 and np.array_equal(n["ref"], g["ref"])


@pytest.mark.parametrize("style,C,diag", [c for c in PR.POSTERIOR_CASES if c[0] == "impulse"])
def test_impulse_keep_decisions_stay_clear_of_the_weights_own_error(style, C, diag):
    """the condition of the GPU test: at most 1 % of the (sample, pixel) pairs have |u - w| inside 4x the fp32 mirror's own error in w
    (floor 1e-6); the expected count is below 1 of 560"""
    _, m, fig, model = PR.posterior_case(style, C, diag)
    band = max(1e-6, 4 * fig["w"])
    near = np.abs(model["u"].astype(np.float64) - m["w"].numpy()[None]) <= band
    print("band %.2e: %d of %d pairs inside" % (band, int(near.sum()), near.size))
    assert near.size == 560 and int(near.sum()) * 100 <= near.size
    keep = model["u"].astype(np.float64) < m["w"].numpy()[None]
    assert 0 < int(keep.sum()) < keep.size                       # both components occur


def test_posterior_sample_model_factors_reproduce_the_covariance():
    """L L^T (U U^T) of the factor the model is given is the mirror's covariance (prior covariance)"""
    from posterior_ref import full_matrix
    for style, C, diag in PR.POSTERIOR_CASES:
        (no, y, npar, est), m, fig, model = PR.posterior_case(style, C, diag)
        assert model["samples"].shape == (PR.POSTERIOR_S, PR.POSTERIOR_B, C, PR.POSTERIOR_H, PR.POSTERIOR_W) and np.isfinite(model["samples"]).all()
        ctr = (m["prior_mean"] if style == "impulse" else m["mean"]).numpy()
        cov = full_matrix(m["prior_cov"] if style == "impulse" else m["cov"]).numpy()
        x = model["drawn"] if style == "impulse" else model["samples"]
        d = np.moveaxis(x - ctr[None], 2, -1)                                   # [S,B,H,W,C] = F z
        zz = np.moveaxis(model["z"], 2, -1)
        # F from the samples: solve nothing, just check the Mahalanobis identity d^T Sigma^-1 d = z^T z where Sigma is well conditioned
        ev = np.linalg.eigvalsh(cov)
        ok = ev[..., 0] > 1e-9 * ev[..., -1].max()
        q = np.einsum("sbhwi,bhwij,sbhwj->sbhw", d, np.linalg.inv(np.where(ok[..., None, None], cov, np.eye(C))), d)
        np.testing.assert_allclose(q[:, ok], (zz * zz).sum(-1)[:, ok], rtol=1e-6)
        assert int(ok.sum()) * 2 > ok.size
