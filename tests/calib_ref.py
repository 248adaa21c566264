"""Calibration quantities that share no code with the package: per-pixel Mahalanobis distance, log-determinant and z-scores through
numpy.linalg (float64), and the (mean, cov, ref) triples the calibration tests run on.

The triples are built so that exact comparisons of counts are legitimate: `make_inputs` itself asserts that every covariance has a
condition number of at most 1e4, that no |z_c| lies within 1e-9 (relative) of 1, 2, 3 or of a histogram edge, that no d^2 lies within 1e-9
of a chi^2 threshold and that no pixel is degenerate.  A count can then differ between two correct float64 evaluations only if a value
moves by more than ~1e4 * 2^-53 * a few operations ~ 1e-11 relative: it cannot.  A seed that violates one of these is replaced, the bound
stays."""
import numpy as np
import torch

CHI2 = {1: (0.45493642311957, 2.70554345409541, 6.63489660102120), 3: (2.36597388437534, 6.25138863117032, 11.3448667301444)}
EDGES = np.array([-4.0 + 0.25 * k for k in range(33)])       # the 33 edges of the 32 inner histogram bins
TRI = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))       # SSDN_OP_HEAD_POSTERIOR's order of the upper triangle
COND_MAX, NEAR = 1e4, 1e-9


def full_cov(cov):
    """cov [B, C(C+1)/2, H, W] -> float64 numpy [B,H,W,C,C]"""
    cov = np.asarray(cov, dtype=np.float64)
    B, K, H, W = cov.shape
    C = 1 if K == 1 else 3
    S = np.zeros((B, H, W, C, C))
    for k, (i, j) in enumerate(TRI[:K] if C == 3 else ((0, 0),)):
        S[..., i, j] = S[..., j, i] = cov[:, k]
    return S


def calib_numpy(mean, cov, ref):
    """-> (d2 [B,H,W], logdet [B,H,W], z [B,C,H,W]) float64 numpy: r^T S^-1 r by numpy.linalg.solve, ln det S by numpy.linalg.slogdet"""
    S = full_cov(cov)
    r = np.moveaxis(np.asarray(ref, dtype=np.float64) - np.asarray(mean, dtype=np.float64), 1, -1)          # [B,H,W,C]
    d2 = np.einsum("bhwc,bhwc->bhw", r, np.linalg.solve(S, r[..., None])[..., 0])
    sign, logdet = np.linalg.slogdet(S)
    assert (sign > 0).all()
    z = r / np.sqrt(np.einsum("bhwcc->bhwc", S))
    return d2, logdet, np.moveaxis(z, -1, 1)


def make_inputs(B, C, H, W, seed=0):
    """(mean, cov, ref) float32 torch tensors.  mean: uniform in [0.25, 0.75]; cov = A A^T + delta I per pixel with the entries of A
    uniform in (-a, a), a log-uniform in [0.01, 0.1] per pixel, delta = a^2 / 50, so the entries lie in 1e-4 ... 1e-2 and the condition
    number is below 3 * 3 a^2 / delta + 1 = 451; ref = mean + L g clipped to [0, 1] with g standard normal, so the z-scores and d^2 spread
    over all the thresholds the statistics count against.  All rounded to float32 first; the assertions are made on the rounded values."""
    rng = np.random.default_rng(4000 + seed)
    mean = rng.uniform(0.25, 0.75, (B, C, H, W)).astype(np.float32)
    a = np.exp(rng.uniform(np.log(0.01), np.log(0.1), (B, H, W, 1, 1)))
    A = rng.uniform(-1, 1, (B, H, W, C, C)) * a
    S = A @ np.swapaxes(A, -1, -2) + (a * a / 50) * np.eye(C)
    idx = TRI if C == 3 else ((0, 0),)
    cov = np.stack([S[..., i, j] for i, j in idx], 1).astype(np.float32)
    L = np.linalg.cholesky(full_cov(cov))
    g = rng.standard_normal((B, H, W, C, 1))
    ref = np.clip(mean.astype(np.float64) + np.moveaxis((L @ g)[..., 0], -1, 1), 0, 1).astype(np.float32)
    # the conditions that make exact comparisons legitimate
    ev = np.linalg.eigvalsh(full_cov(cov))
    assert (ev[..., 0] > 0).all() and float((ev[..., -1] / ev[..., 0]).max()) <= COND_MAX, "condition number"
    assert np.isfinite(mean).all() and np.isfinite(cov).all() and np.isfinite(ref).all()
    d2, _, z = calib_numpy(mean, cov, ref)
    for k in (1.0, 2.0, 3.0):
        assert (np.abs(np.abs(z) - k) > NEAR * k).all(), "a |z| too close to %g" % k
    for e in EDGES:
        assert (np.abs(z - e) > NEAR * max(abs(e), 1.0)).all(), "a z too close to the histogram edge %g" % e
    for q in CHI2[C]:
        assert (np.abs(d2 - q) > NEAR * q).all(), "a d2 too close to the chi^2 threshold %g" % q
    return torch.from_numpy(mean), torch.from_numpy(cov), torch.from_numpy(ref)
