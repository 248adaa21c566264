"""The library's random streams as an exact host model (numpy; no torch on the random path): Philox4x32-10, the map of a random word to
(0, 1] and the Box-Muller normals of csrc/philox.h, SSDN_OP_NOISE (csrc/elementwise.hip: k_noise, k_noise_impulse) element by element, and
the sample loop of SSDN_OP_HEAD_POSTERIOR (csrc/head_posterior.hip).  Everything is restated from those files, not from the reference
package: the counter layouts, the stream ids, the Poisson inversion with its float32 thresholds, the Noise2Void draws.

What is exact and what is not.  Integer arithmetic and every float32 operation that is ONE correctly rounded operation in the kernel
(u01: the multiply by 2^-24 is exact, so fused or not it is one rounding; u8 / 255; u * span) give the kernel's bits.  The normals are
evaluated in float64 on the float32 u01 values: the kernel's __logf / __cosf / __sinf are approximations, so a draw is compared within a
tolerance in units of one standard normal (Z_TOL).  A float comparison that one ulp could turn (u01 against a Poisson threshold or against
a ranged alpha, which the kernel may form with or without a fused multiply-add) is reported in `fragile`; the cases below are chosen so
that no element is fragile and the GPU tests exclude nothing (tests/test_philox_ref_cpu.py asserts it)."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
NS_INPUT, NS_REF, NS_PARAM, NS_COORD, NS_PARAM_REF = 0, 1, 2, 3, 4          # elementwise.hip
PH_STREAM_POSTERIOR = 0x80000000                                            # philox.h
TWO_PI_F32 = float(np.float32(6.28318530718))                               # the kernel's constant, as fp32 holds it
FRAGILE = 2.0 ** -22
# Draw identity, in units of one standard normal.  Derived, not measured: the kernel's only approximations are __logf, __cosf and __sinf;
# the worst case is the total loss of the logarithm at u = 1 - 2^-24, which changes sqrt(-2 ln u) by 3.5e-4.  A WRONG draw is an
# independent normal and lands within 1e-3 of the right one with probability below 6e-4 per element.
Z_TOL = 1e-3


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Random123), vectorised: uint64 arithmetic masked to 32 bits; ten rounds, the key bumped after each (the tenth bump
    is unused, as in the kernel).  -> four uint64 arrays holding 32-bit words"""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(_u64(c0), _u64(c1), _u64(c2), _u64(c3), _u64(k0), _u64(k1))
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & M32, p1 >> np.uint64(32), p1 & M32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def u01(x):
    """float32, the kernel's expression: (float)(x >> 8) * 2^-24 + 2^-25.  The range is (0, 1]: u01(0xFFFFFFFF) rounds up to 1.0"""
    return (_u64(x) >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24) + np.float32(2.0 ** -25)


def _polar(a, b):
    return np.sqrt(-2.0 * np.log(u01(a).astype(np.float64))), TWO_PI_F32 * u01(b).astype(np.float64)


def normal(a, b):
    """ph_normal: Box-Muller, the cosine branch; float64 on the float32 u01 values"""
    r, t = _polar(a, b)
    return r * np.cos(t)


def normal2(a, b):
    """ph_normal2: the cosine, then the sine branch of the same two words"""
    r, t = _polar(a, b)
    return r * np.cos(t), r * np.sin(t)


def _words(seed, offset):
    seed, offset = int(seed), int(offset)
    return offset & 0xFFFFFFFF, offset >> 32, seed & 0xFFFFFFFF, seed >> 32         # counter words 2, 3; key words 0, 1


def _draw(counter, stream, seed, offset):
    o0, o1, k0, k1 = _words(seed, offset)
    return philox4x32_10(counter, stream, o0, o1, k0, k1)


def poisson_thresholds():
    """the cdf values noise_apply compares u with, float32: T[0] = pk = 0.36787944117f, then pk /= k, cdf += pk for k = 1 .. 16.  The loop
    `while (u > cdf && k < 16)` looks at T[0] .. T[15]"""
    pk = np.float32(0.36787944117)
    cdf = pk
    t = [cdf]
    for k in range(1, 17):
        pk = np.float32(pk / np.float32(k))
        cdf = np.float32(cdf + pk)
        t.append(cdf)
    return np.array(t, dtype=np.float32)


def poisson1(u):
    """Poisson(1) by inversion, the kernel's loop on a float32 u -> (k, fragile).  The thresholds do not decrease, so the loop's k is the
    number of T[0] .. T[15] below u"""
    t = poisson_thresholds()[:16]
    u = np.asarray(u, dtype=np.float32)
    k = (u[..., None] > t).sum(-1)
    fragile = (np.abs(u[..., None].astype(np.float64) - t.astype(np.float64)) < FRAGILE).any(-1)
    return k, fragile


def n2v_pick(c, r, size, u):
    """n2v_pick of elementwise.hip: a uniform integer over [min(c - r, 0), min(c + r, size - 1)) without c, from a float32 u (scalar or
    array) through the float32 product u * span; a negative result wraps (Python indexing)"""
    lo, hi = min(c - r, 0), min(c + r, size - 1)
    inside = lo <= c < hi
    span = max(hi - lo - (1 if inside else 0), 1)
    k = (np.asarray(u, dtype=np.float32) * np.float32(span)).astype(np.int64)         # (int): truncation, the product is not negative
    k = np.minimum(k, span - 1)
    v = lo + k
    if inside:
        v = np.where(v >= c, v + 1, v)
    v = np.where(v < 0, v + size, v)
    return np.minimum(v, size - 1)


def _param(bc, stream, p_lo, p_hi, seed, offset):
    """noise_param: fixed -> float32 exactly; ranged -> p_lo + (p_hi - p_lo) * u01 in float64 on the float32 operands (the kernel may fuse
    the two operations or not: within 2^-22 relative of either)"""
    lo, hi = np.float32(p_lo), np.float32(p_hi)
    if lo == hi:
        return np.full(np.shape(bc), lo, dtype=np.float64)
    u = u01(_draw(bc, stream, seed, offset)[0])
    return float(lo) + float(np.float32(hi - lo)) * u.astype(np.float64)


def _apply(style, clip, clean, param, e, stream, seed, offset):
    """noise_apply on arrays: clean float32, param float64, e the element counters -> (value float64, z or k, fragile)"""
    w = _draw(e, stream, seed, offset)
    c64 = clean.astype(np.float64)
    if style == 0:
        aux = normal(w[0], w[1])
        v, fragile = c64 + param * aux, np.zeros(np.shape(e), dtype=bool)
    else:
        aux, fragile = poisson1(u01(w[0]))
        v = (c64 * param + aux) / param
    if clip:
        v = np.clip(v, 0.0, 1.0)
    return v, aux, fragile


def noise_model(u8, style, clip, p_lo, p_hi, seed, offset, ref=True, n2v_box=0, n2v_radius=2):
    """SSDN_OP_NOISE on a [B,C,H,W] uint8 array -> dict of clean (float32, exact), noisy, ref, param [B,C], param_ref (float64), coords
    [B, cells, 2] int64 (None without n2v_box), fragile [B,C,H,W] bool, and what the tests read besides: `draw` / `draw_ref` (z of gauss,
    k of poisson, the hit mask of impulse, per element of the UNMANIPULATED realisation) and `src` [B, cells, 2] = the drawn (rx, ry).
    Counters: element bc HW + y W + x (gauss, poisson), pixel b HW + y W + x (impulse), bc for a parameter (impulse: b C for all
    channels), the cell index b cells + i (H / box) + j for coordinates; counter words (., stream, offset lo, offset hi), key (seed lo,
    seed hi)."""
    u8 = np.ascontiguousarray(np.asarray(u8, dtype=np.uint8))
    B, C, H, W = u8.shape
    HW = H * W
    clean = u8.astype(np.float32) / np.float32(255)
    ranged = np.float32(p_lo) != np.float32(p_hi)
    bc = np.arange(B * C).reshape(B, C)
    if style == 2:
        bc = np.broadcast_to((np.arange(B) * C)[:, None], (B, C))                  # one alpha per sample, in all C entries
    param = _param(bc, NS_PARAM, p_lo, p_hi, seed, offset)
    param_ref = _param(bc, NS_PARAM_REF, p_lo, p_hi, seed, offset) if ref else None
    out = dict(clean=clean, param=param, param_ref=param_ref, coords=None, src=None, ref=None, draw_ref=None)
    if style == 2:
        px = np.arange(B * HW).reshape(B, 1, H, W)

        def realise(stream, alpha):
            w = _draw(px, stream, seed, offset)
            u, a = u01(w[0]), alpha[:, :1, None, None]
            # a fixed alpha is compared in float32, bit for bit; a ranged one within the band its two possible roundings leave
            hit = (u < np.float32(p_lo)) if not ranged else (u.astype(np.float64) < a)
            fragile = np.zeros(u.shape, dtype=bool) if not ranged else np.abs(u.astype(np.float64) - a) < FRAGILE
            colour = np.concatenate([u01(w[1 + c]) for c in range(C)], 1)        # word 0 decides, words 1 .. 3 are the colour
            return np.where(hit, colour, clean).astype(np.float64), np.broadcast_to(hit, (B, C, H, W)), np.broadcast_to(fragile, (B, C, H, W))
        noisy, draw, fragile = realise(NS_INPUT, param)
        if ref:
            out["ref"], out["draw_ref"], fr = realise(NS_REF, param_ref)
            fragile = fragile | fr
    else:
        e = np.arange(B * C * HW).reshape(B, C, H, W)
        noisy, draw, fragile = _apply(style, clip, clean, param[:, :, None, None], e, NS_INPUT, seed, offset)
        if ref:
            out["ref"], out["draw_ref"], fr = _apply(style, clip, clean, param_ref[:, :, None, None], e, NS_REF, seed, offset)
            fragile = fragile | fr
    out["draw"] = draw
    if n2v_box > 0:
        box, n0, n1 = n2v_box, W // n2v_box, H // n2v_box
        coords, src = np.zeros((B, n0 * n1, 2), dtype=np.int64), np.zeros((B, n0 * n1, 2), dtype=np.int64)
        plain, noisy = noisy, noisy.copy()
        for b in range(B):
            for i in range(n0):
                for j in range(n1):
                    cell = i * n1 + j
                    w = [int(v) for v in _draw(b * n0 * n1 + cell, NS_COORD, seed, offset)]
                    c0 = min(i * box + int(u01(w[0]) * np.float32(box)), i * box + box - 1)
                    c1 = min(j * box + int(u01(w[1]) * np.float32(box)), j * box + box - 1)
                    rx, ry = int(n2v_pick(c0, n2v_radius, W, u01(w[2]))), int(n2v_pick(c1, n2v_radius, H, u01(w[3])))
                    coords[b, cell], src[b, cell] = (c0, c1), (rx, ry)
                    # the replaced pixel holds the noisy value of element (ry, rx), derived from THAT element's counter with this channel's
                    # parameter: exactly the unmanipulated realisation there (impulse: its source pixel's decision and colour)
                    noisy[b, :, c1, c0] = plain[b, :, ry, rx]
        out["coords"], out["src"] = coords, src
    out["noisy"], out["fragile"] = noisy, np.ascontiguousarray(fragile)
    return out


def posterior_samples_model(ctr, factor, kind, w, y, B, H, W, S, seed, offset):
    """the sample loop of k_head_posterior<*, true>.  ctr [B,C,H,W]: the centre (posterior mean; impulse: mu_x); factor [B,C(C+1)/2,H,W]
    in Sym3 order: kind "gauss": the LOWER triangular L (l00, l10, l20, l11, l21, l22), x = ctr + L z; kind "impulse": the UPPER
    triangular U of net_out (u00, u01, u02, u11, u12, u22), x = y where u01 < w [B,H,W], else ctr + U z.  Sample s of pixel e0 = b HW + p
    draws from stream 0x80000000 + 2 s (z0, z1 = normal2(v0, v1), z2 = normal(v2, v3); C = 1: normal(v0, v1)) and + 2 s + 1 (word 0: the
    keep decision).  -> dict: samples [S,B,C,H,W] float64, z [S,B,C,H,W], and for impulse u [S,B,H,W] float32 (`samples` then takes the
    model's own decision u < w; `drawn` is ctr + U z everywhere)"""
    ctr, f = np.asarray(ctr, dtype=np.float64), np.asarray(factor, dtype=np.float64)
    C = ctr.shape[1]
    e0 = np.arange(B * H * W).reshape(1, B, H, W)
    s = np.arange(S).reshape(S, 1, 1, 1)
    v = _draw(e0, PH_STREAM_POSTERIOR + 2 * s, seed, offset)
    if C == 1:
        z = normal(v[0], v[1])[:, :, None]
        x = ctr[None] + f[None] * z
    else:
        z0, z1 = normal2(v[0], v[1])
        z2 = normal(v[2], v[3])
        z = np.stack([z0, z1, z2], 2)
        if kind == "impulse":
            rows = [f[:, 0] * z0 + f[:, 1] * z1 + f[:, 2] * z2, f[:, 3] * z1 + f[:, 4] * z2, f[:, 5] * z2]
        else:
            rows = [f[:, 0] * z0, f[:, 1] * z0 + f[:, 3] * z1, f[:, 2] * z0 + f[:, 4] * z1 + f[:, 5] * z2]
        x = ctr[None] + np.stack(rows, 2)
    out = dict(samples=x, z=z)
    if kind == "impulse":
        u = u01(_draw(e0, PH_STREAM_POSTERIOR + 2 * s + 1, seed, offset)[0])
        keep = u.astype(np.float64) < np.asarray(w, dtype=np.float64)[None]
        out.update(u=u, drawn=x, samples=np.where(keep[:, :, None], np.asarray(y, dtype=np.float64)[None], x))
    return out


# ---- the cases of the GPU tests (tests/test_hip_random_streams.py); tests/test_philox_ref_cpu.py asserts on the model alone that none of
# them has a fragile element.  Both high words carry information.
SEED, OFFSET = (5 << 32) | 7, (3 << 32) | 9
SEED_HI, OFFSET_HI = (6 << 32) | 7, (4 << 32) | 9              # differ from SEED / OFFSET in the high word ONLY
B, H, W = 2, 24, 40                                            # non-square, 3 x 5 Noise2Void boxes, 1920 threads, <= 5760 elements
GAUSS, POISSON, IMPULSE = (25 / 255.0, 25 / 255.0), (30.0, 30.0), (0.5, 0.5)
GAUSS_R, POISSON_R, IMPULSE_R = (5 / 255.0, 50 / 255.0), (5.0, 50.0), (0.2, 0.4)
# (style, clip, p_lo, p_hi)
GAUSS_CASES = [(0, clip, lo, hi) for (lo, hi) in (GAUSS, GAUSS_R) for clip in (True, False)]
POISSON_CASES = [(1, clip, lo, hi) for (lo, hi) in (POISSON, POISSON_R) for clip in (True, False)]
IMPULSE_CASES = [(2, False, lo, hi) for (lo, hi) in ((0.05, 0.05), IMPULSE, IMPULSE_R)]
N2V_CASES = [(0, True) + GAUSS_R, (1, False) + POISSON, (2, False) + IMPULSE_R]
# DevicePatchStream: seed s, rank r -> key s + r = SEED; the n-th prepare is offset n
STREAM_SEED, STREAM_RANK, STREAM_CALLS = SEED - 4, 4, 3
# (noise style, algorithm, the op's (style, clip, p_lo, p_hi), Noise2Void manipulation)
STREAM_CASES = [("gauss5_50", "NOISE_TO_NOISE", (0, True) + GAUSS_R, False), ("poisson30", "NOISE_TO_VOID", (1, True) + POISSON, True)]
# SSDN_OP_HEAD_POSTERIOR samples: (style, C, diag), mode "known", op_inputs(..., H=5, W=7), B = 2, S = 8
POSTERIOR_CASES = [("gauss25", 3, 0), ("gauss25", 3, 1), ("poisson30", 1, 0), ("impulse", 3, 0), ("impulse", 1, 0)]
POSTERIOR_B, POSTERIOR_H, POSTERIOR_W, POSTERIOR_S = 2, 5, 7, 8


def case_image(C, seed=0):
    """the random uint8 images [B,C,H,W] of the noise cases"""
    return np.random.RandomState(1000 + 10 * seed + C).randint(0, 256, (B, C, H, W)).astype(np.uint8)


def all_noise_runs():
    """every (C, style, clip, lo, hi, seed, offset, n2v) the GPU tests launch"""
    runs = []
    for C in (3, 1):
        runs += [(C,) + c + (SEED, OFFSET, False) for c in GAUSS_CASES + POISSON_CASES + IMPULSE_CASES]
        runs += [(C,) + c + (SEED, OFFSET, True) for c in N2V_CASES]
    for sd, off in ((SEED, OFFSET_HI), (SEED_HI, OFFSET)):
        runs += [(3,) + c + (sd, off, True) for c in N2V_CASES]
    for n in range(STREAM_CALLS):
        runs += [(3,) + c + (STREAM_SEED + STREAM_RANK, n, n2v) for _, _, c, n2v in STREAM_CASES]
    return runs


def posterior_case(style, C, diag, seed=SEED, offset=OFFSET):
    """one POSTERIOR_CASES entry -> (inputs (net_out, noisy, npar, est), the float64 mirror, its fp32 yardstick, the sample model): the
    centre, the covariance and the impulse weight come from tests/posterior_ref.py; L is numpy's Cholesky factor of the mirror's float64
    covariance (diagonal head, C = 1: the square roots), the impulse factor is U itself from net_out"""
    from posterior_ref import fp32_yardstick, full_matrix, is_impulse, op_inputs, posterior_ref
    Bp, Hp, Wp, S = POSTERIOR_B, POSTERIOR_H, POSTERIOR_W, POSTERIOR_S
    inputs = no, y, npar, est = op_inputs(style, "known", C, diag, B=Bp, H=Hp, W=Wp)
    m = posterior_ref(no, y, npar, style, "known", est, diag)
    fig = fp32_yardstick(no, y, npar, style, "known", est, diag, m)
    if is_impulse(style):
        model = posterior_samples_model(m["prior_mean"].numpy(), no[:, C:].double().numpy(), "impulse", m["w"].numpy(), y.double().numpy(),
                                        Bp, Hp, Wp, S, seed, offset)
    else:
        cov = m["cov"].numpy()
        if C == 1:
            factor = np.sqrt(np.maximum(cov, 0.0))
        elif diag:
            factor = np.where(np.array([1, 0, 0, 1, 0, 1], dtype=bool)[None, :, None, None], np.sqrt(np.maximum(cov, 0.0)), 0.0)
        else:
            L = np.linalg.cholesky(full_matrix(m["cov"]).numpy())
            factor = np.stack([L[..., i, j] for (j, i) in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))], 1)
        model = posterior_samples_model(m["mean"].numpy(), factor, "gauss", None, None, Bp, Hp, Wp, S, seed, offset)
    return inputs, m, fig, model
