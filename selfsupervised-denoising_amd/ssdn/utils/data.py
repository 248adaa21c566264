"""Tensor helpers used on / next to the hot path (drop-in for the used part of /root/reference/ssdn/ssdn/utils/data.py)."""
import math
from typing import Dict

import torch
from torch import Tensor


def clip_img(img: Tensor, inplace: bool = False) -> Tensor:
    """Clamp to the valid image range: [0,1] for float images, [0,255] for integer images (utils/data.py:19-39)."""
    if not inplace:
        img = img.clone()
    hi = 1 if img.is_floating_point() else 255
    return img.clamp_(0, hi)


def rotate(x: Tensor, angle: int) -> Tensor:
    """BCHW rotation in multiples of 90 degrees with the reference's NUMERIC convention (utils/data.py:42-67):
    rotate(x, 90)[i, j] = x[j, W-1-i] (counter-clockwise although documented clockwise).  On the device the rotations are
    never materialised by this function -- SSDN_OP_PACK_INPUT / SSDN_OP_UNROT_* fold them into loads; this host version
    exists for API parity and tests."""
    if angle == 0:
        return x
    if angle == 90:
        return x.flip(-1).transpose(-2, -1)
    if angle == 180:
        return x.flip(-1).flip(-2)
    if angle == 270:
        return x.flip(-2).transpose(-2, -1)
    raise NotImplementedError("Must be rotation divisible by 90 degrees")


def mse2psnr(mse: Tensor, float_imgs: bool = True) -> Tensor:
    peak = 1.0 if float_imgs else 255.0
    return 20 * torch.log10(torch.tensor(peak, device=mse.device)) - 10 * torch.log10(mse)


def calculate_psnr(img: Tensor, ref: Tensor) -> Tensor:
    """Per-sample PSNR for BCHW (or a single CHW image): -10 log10(mean_chw (img-ref)^2) (utils/data.py:94-105)."""
    se = (img - ref) ** 2
    mse = se.reshape(se.shape[0], -1).mean(1) if se.dim() == 4 else se.mean()
    return mse2psnr(mse, img.is_floating_point())


SSIM_WIN, SSIM_SIGMA, SSIM_C1, SSIM_C2 = 11, 1.5, 0.01 ** 2, 0.03 ** 2


def ssim_window(device=None) -> Tensor:
    """g[k] ~ exp(-(k - 5)^2 / (2 * 1.5^2)), k = 0..10, normalised to sum 1 (float64)"""
    k = torch.arange(SSIM_WIN, dtype=torch.float64, device=device) - SSIM_WIN // 2
    g = torch.exp(-(k * k) / (2 * SSIM_SIGMA ** 2))
    return g / g.sum()


def calculate_ssim(img: Tensor, ref: Tensor, full: bool = False):
    """Per-sample SSIM for BCHW (or a single CHW image) -- the specification SSDN_OP_SSIM (csrc/ssim.hip) is held to, in float64.
    Wang, Bovik, Sheikh, Simoncelli 2004 with the parameters of the authors' code (scikit-image: gaussian_weights=True,
    use_sample_covariance=False, data_range=1): an 11 x 11 separable Gaussian window of sd 1.5 at the positions where it lies wholly
    inside the image (no padding), C1 = 0.01^2, C2 = 0.03^2, the raw float images (nothing is clipped, as in calculate_psnr); the
    value is the plain mean over channels and positions, NaN for an image below 11 pixels in either axis.  Returns float32 like
    calculate_psnr ([B], or a scalar for CHW); full=True: (that, the float64 map [B, C, H - 10, W - 10] / [C, H - 10, W - 10])."""
    import torch.nn.functional as F
    single = img.dim() == 3
    x = (img[None] if single else img).to(torch.float64)
    y = (ref[None] if single else ref).to(torch.float64)
    if x.dim() != 4 or x.shape != y.shape:
        raise ValueError("calculate_ssim: two BCHW (or CHW) images of one shape, got %s and %s" % (tuple(img.shape), tuple(ref.shape)))
    B, C, H, W = x.shape
    if H < SSIM_WIN or W < SSIM_WIN:
        val = torch.full((B,), float("nan"), dtype=torch.float32, device=x.device)
        smap = torch.zeros((B, C, max(H - SSIM_WIN + 1, 0), max(W - SSIM_WIN + 1, 0)), dtype=torch.float64, device=x.device)
    else:
        g = ssim_window(x.device)

        def win(t):                  # E[t]: 11 taps along the rows, then 11 down the columns, every plane on its own
            t = t.reshape(B * C, 1, H, W)
            t = F.conv2d(F.conv2d(t, g.view(1, 1, 1, -1)), g.view(1, 1, -1, 1))
            return t.reshape(B, C, H - SSIM_WIN + 1, W - SSIM_WIN + 1)
        mx, my = win(x), win(y)
        sxx, syy, sxy = win(x * x) - mx * mx, win(y * y) - my * my, win(x * y) - mx * my
        smap = ((2 * mx * my + SSIM_C1) * (2 * sxy + SSIM_C2)) / ((mx * mx + my * my + SSIM_C1) * (sxx + syy + SSIM_C2))
        val = smap.reshape(B, -1).mean(1).to(torch.float32)
    if single:
        val, smap = val[0], smap[0]
    return (val, smap) if full else val


# the chi^2_C quantiles at 0.5, 0.9 and 0.99 (C = 1: erf(sqrt(x/2)) = p; C = 3: erf(sqrt(x/2)) - sqrt(2x/pi) exp(-x/2) = p) and the
# nominal levels the counts of |z| <= 1, 2, 3 are judged against, erf(k / sqrt 2)
CALIB_CHI2_LEVELS = (0.5, 0.9, 0.99)
CALIB_CHI2 = {1: (0.45493642311957, 2.70554345409541, 6.63489660102120), 3: (2.36597388437534, 6.25138863117032, 11.3448667301444)}
CALIB_SIGMA_LEVELS = (0.6826894921370859, 0.9544997361036416, 0.9973002039367398)
CALIB_NSTATS, CALIB_HIST_BINS = 12, 34
CALIB_VALUES = ("nll", "maha", "rmse_ratio", "cover_1s", "cover_2s", "cover_3s", "cover_50", "cover_90", "cover_99", "degenerate")


def calibration_values(stats: Tensor, channels: int) -> Dict[str, Tensor]:
    """The reported calibration values from the raw statistics [..., 12] (float64) of calculate_calibration / SSDN_OP_CALIBRATION:
    nll = (sum d2 + sum logdet) / (2 N C) + ln(2 pi) / 2 (nats per pixel-channel of the clean image under the posterior), maha =
    sum d2 / (N C) (ideal 1; above 1 the model is over-confident), rmse_ratio = sqrt(sum |r|^2 / sum tr S) (actual over predicted RMSE),
    cover_1s/2s/3s = counts / (N C), cover_50/90/99 = counts / N, degenerate = degenerate / (N + degenerate).  N = 0: the ratios are NaN."""
    s = stats.to(torch.float64)
    nan = torch.full_like(s[..., 0], float("nan"))
    n, deg = s[..., 0], s[..., 1]
    some = n > 0
    nc = torch.where(some, n * channels, nan)
    res = {"nll": 0.5 * (s[..., 2] + s[..., 3]) / nc + 0.5 * math.log(2 * math.pi), "maha": s[..., 2] / nc,
           "rmse_ratio": torch.where(some, torch.sqrt(s[..., 4] / torch.where(some, s[..., 5], nan)), nan)}
    for k, name in enumerate(("cover_1s", "cover_2s", "cover_3s")):
        res[name] = s[..., 6 + k] / nc
    for k, name in enumerate(("cover_50", "cover_90", "cover_99")):
        res[name] = s[..., 9 + k] / torch.where(some, n, nan)
    res["degenerate"] = torch.where(n + deg > 0, deg / torch.where(n + deg > 0, n + deg, nan), nan)
    return res


def calculate_calibration(mean: Tensor, cov: Tensor, ref: Tensor, hist: bool = False, zmap: bool = False) -> Dict[str, Tensor]:
    """Per-sample calibration of a per-pixel Gaussian posterior N(mean, S) against the clean image -- the specification
    SSDN_OP_CALIBRATION (csrc/calibration.hip) is held to, float64 on any device.  mean, ref: [B,C,H,W]; cov: [B, C(C+1)/2, H, W] in
    SSDN_OP_HEAD_POSTERIOR's order (00, 01, 02, 11, 12, 22; C = 1: the variance), C in {1, 3}; the caller crops to the un-padded
    extent, as with calculate_ssim.  Per pixel, in float64 from the inputs as they are, r = ref - mean and, in this fixed order (C = 3),
        p0 = s00, l00 = sqrt p0, l10 = s01 / l00, l20 = s02 / l00;  p1 = s11 - l10^2, l11 = sqrt p1, l21 = (s12 - l20 l10) / l11;
        p2 = s22 - l20^2 - l21^2, l22 = sqrt p2;  w0 = r0 / l00, w1 = (r1 - l10 w0) / l11, w2 = (r2 - l20 w0 - l21 w1) / l22;
        d2 = w0^2 + w1^2 + w2^2, logdet = ln p0 + ln p1 + ln p2   (C = 1: d2 = r^2 / s, logdet = ln s),   z_c = r_c / sqrt(s_cc).
    A pixel is valid iff all its inputs are finite, every pivot p_k > 0 and every s_cc > 0; a degenerate pixel is counted and left out
    of everything else.  -> {"stats": float64 [B,12]: N, degenerate, sum d2, sum logdet, sum |r|^2, sum tr S, the (valid pixel, channel)
    pairs with |z_c| <= 1, 2, 3, the valid pixels with d2 <= the chi^2_C quantile at 0.5, 0.9, 0.99 (CALIB_CHI2)} and the values
    `calibration_values` derives from them, float64 [B] each.  hist=True adds "hist", int64 [B,C,34]: counts of z_c over the valid
    pixels (bin 0: z < -4; bin 1 + floor(4 z + 16): -4 <= z < 4; bin 33: z >= 4); zmap=True adds "zmap", float64 [B,C,H,W], NaN at
    degenerate pixels.
    For an impulse model the posterior is a two-component mixture and `cov` its moment-matched covariance (Denoiser.posterior): the
    statistics describe that Gaussian, not the mixture."""
    if mean.dim() != 4 or mean.shape != ref.shape or mean.shape[1] not in (1, 3):
        raise ValueError("calculate_calibration: mean and ref must be BCHW of one shape with C in {1, 3}, got %s and %s"
                         % (tuple(mean.shape), tuple(ref.shape)))
    B, C, H, W = mean.shape
    if tuple(cov.shape) != (B, C * (C + 1) // 2, H, W):
        raise ValueError("calculate_calibration: cov must be %s, got %s" % ((B, C * (C + 1) // 2, H, W), tuple(cov.shape)))
    m, s, y = mean.to(torch.float64), cov.to(torch.float64), ref.to(torch.float64)
    fin = torch.isfinite(m).all(1) & torch.isfinite(s).all(1) & torch.isfinite(y).all(1)
    r = y - m
    if C == 3:
        r0, r1, r2 = r[:, 0], r[:, 1], r[:, 2]
        s00, s01, s02, s11, s12, s22 = (s[:, k] for k in range(6))
        p0 = s00
        l00 = torch.sqrt(p0)
        l10, l20 = s01 / l00, s02 / l00
        p1 = s11 - l10 * l10
        l11 = torch.sqrt(p1)
        l21 = (s12 - l20 * l10) / l11
        p2 = (s22 - l20 * l20) - l21 * l21
        l22 = torch.sqrt(p2)
        w0 = r0 / l00
        w1 = (r1 - l10 * w0) / l11
        w2 = ((r2 - l20 * w0) - l21 * w1) / l22
        d2 = (w0 * w0 + w1 * w1) + w2 * w2
        logdet = (torch.log(p0) + torch.log(p1)) + torch.log(p2)
        valid = fin & (p0 > 0) & (p1 > 0) & (p2 > 0) & (s11 > 0) & (s22 > 0)
        rr = (r0 * r0 + r1 * r1) + r2 * r2
        tr = (s00 + s11) + s22
        z = torch.stack([r0 / torch.sqrt(s00), r1 / torch.sqrt(s11), r2 / torch.sqrt(s22)], 1)
    else:
        r0, s00 = r[:, 0], s[:, 0]
        valid = fin & (s00 > 0)
        d2 = (r0 * r0) / s00
        logdet = torch.log(s00)
        rr, tr = r0 * r0, s00
        z = (r0 / torch.sqrt(s00))[:, None]
    zero = torch.zeros((), dtype=torch.float64, device=m.device)

    def total(v):                       # over the valid pixels of each sample
        return torch.where(valid, v, zero).reshape(B, -1).sum(1)

    def count(mask):
        return mask.reshape(B, -1).sum(1).to(torch.float64)
    vc = valid[:, None]
    az = z.abs()
    cols = [count(valid), count(~valid), total(d2), total(logdet), total(rr), total(tr)]
    cols += [count(vc & (az <= k)) for k in (1.0, 2.0, 3.0)]
    cols += [count(valid & (d2 <= q)) for q in CALIB_CHI2[C]]
    stats = torch.stack(cols, 1)
    res = {"stats": stats}
    res.update(calibration_values(stats, C))
    if hist:
        zz = torch.where(vc, z, zero)
        bins = torch.where(zz < -4.0, torch.zeros_like(zz), torch.where(zz >= 4.0, torch.full_like(zz, CALIB_HIST_BINS - 1),
                                                                        1 + torch.floor(4.0 * zz + 16.0))).to(torch.int64)
        onehot = torch.zeros((B, C, CALIB_HIST_BINS), dtype=torch.int64, device=m.device)
        onehot.scatter_add_(2, bins.reshape(B, C, -1), vc.expand(B, C, H, W).reshape(B, C, -1).to(torch.int64))
        res["hist"] = onehot
    if zmap:
        res["zmap"] = torch.where(vc, z, torch.full_like(z, float("nan")))
    return res


# ---- a reference-free risk estimate (SSDN_OP_RISK, csrc/risk.hip) ----------------------------------------------------------------
RISK_NSTATS = 12
RISK_VALUES = ("mse_mu_est", "mse_out_est", "psnr_mu_est", "psnr_out_est", "mse_mu_se", "mse_out_se", "nll", "weight", "clipped",
               "degenerate")


def risk_values(stats: Tensor, channels: int) -> Dict[str, Tensor]:
    """The reported values from the raw statistics [..., 12] (float64) of calculate_risk / SSDN_OP_RISK.  With N = s0, sum q_mu = s4 - s6
    and sum q_out = s5 + s7:  mse_mu_est = (s4 - s6) / (N C), mse_out_est = (s5 + s7) / (N C): unbiased estimates of the mean squared
    error of the prior mean and of the delivered output against the clean image nobody has;  psnr_*_est = -10 log10 of them, NaN where
    the estimate is <= 0 (it is unbiased, not positive: a small image can give that);  mse_*_se = sqrt((sum q^2 - (sum q)^2 / N) /
    (N (N - 1))) / C, the naive standard error (pixels treated as independent);  nll = (s2 + s3) / (2 N C) + ln(2 pi) / 2, nats per
    pixel-channel of the NOISY image under the model's marginal N(mu_x, Sigma_x + Sigma_n);  weight = s10 / (N C), how much of its own
    noisy value a pixel's output keeps;  clipped = s11 / (N C);  degenerate = s1 / (s0 + s1).  N < 2: the ratios are NaN."""
    s = stats.to(torch.float64)
    nan = torch.full_like(s[..., 0], float("nan"))
    n, deg = s[..., 0], s[..., 1]
    some = n >= 2
    nn = torch.where(some, n, nan)
    nc = nn * channels
    res = {}
    for name, sq, sq2 in (("mu", s[..., 4] - s[..., 6], s[..., 8]), ("out", s[..., 5] + s[..., 7], s[..., 9])):
        mse = sq / nc
        res["mse_%s_est" % name] = mse
        res["psnr_%s_est" % name] = torch.where(mse > 0, -10.0 * torch.log10(torch.where(mse > 0, mse, torch.ones_like(mse))), nan)
        var = (sq2 - sq * sq / nn) / (nn * (nn - 1))
        res["mse_%s_se" % name] = torch.sqrt(torch.clamp(var, min=0.0)) / channels
    res["nll"] = 0.5 * (s[..., 2] + s[..., 3]) / nc + 0.5 * math.log(2 * math.pi)
    res["weight"] = s[..., 10] / nc
    res["clipped"] = s[..., 11] / nc
    res["degenerate"] = torch.where(n + deg > 0, deg / torch.where(n + deg > 0, n + deg, nan), nan)
    return {k: res[k] for k in RISK_VALUES}


def calculate_risk(noisy: Tensor, mu: Tensor, cov_x: Tensor, out: Tensor, noise_var: Tensor, var_hat: Tensor, ext=None, margin: int = 0,
                   maps: bool = False) -> Dict[str, Tensor]:
    """A reference-free estimate of the squared error of a blind-spot model's two outputs -- the specification SSDN_OP_RISK
    (csrc/risk.hip) is held to, float64 on any device.  The prior (mu, Sigma_x) at a pixel depends on the OTHER pixels only and the
    output is affine in the pixel's own noisy value y, out = mu + W (y - mu), W = Sigma_x (Sigma_x + Sigma_n)^-1; for zero-mean noise,
    independent across pixels and channels with variances v_c,
        E|mu - x|^2 = E[ |mu - y|^2 - sum_c v_c ],        E|out - x|^2 = E[ |out - y|^2 + sum_c (2 W_cc - 1) v_c ].
    noisy, mu, out, noise_var (n_c, the model's noise variance), var_hat (v^_c, an unbiased stand-in of v_c): [B,C,H,W]; cov_x:
    [B, C(C+1)/2, H, W], upper triangle 00, 01, 02, 11, 12, 22; C in {1, 3}.  Per pixel, in float64 from the inputs as they are, in this
    fixed order (C = 3), T = Sigma_x + diag(n_c), d = y - mu:
        p0 = t00, l00 = sqrt p0, l10 = t01 / l00, l20 = t02 / l00;  p1 = t11 - l10^2, l11 = sqrt p1, l21 = (t12 - l20 l10) / l11;
        p2 = t22 - l20^2 - l21^2, l22 = sqrt p2;  w0 = d0 / l00, w1 = (d1 - l10 w0) / l11, w2 = (d2 - l20 w0 - l21 w1) / l22;
        d2 = w0^2 + w1^2 + w2^2, logdet = ln p0 + ln p1 + ln p2        (calculate_calibration's spelling, for T);
        Li00 = 1 / l00, Li11 = 1 / l11, Li22 = 1 / l22, Li10 = -(l10 Li00) / l11, Li21 = -(l21 Li11) / l22,
        Li20 = -(l20 Li00 + l21 Li10) / l22;  t00' = Li00^2 + Li10^2 + Li20^2, t11' = Li11^2 + Li21^2, t22' = Li22^2  (diagonal of T^-1);
        W_cc = 1 - n_c t_cc'                     (C = 1: W = 1 - n / (s + n), d2 = d^2 / (s + n), logdet = ln(s + n));
        q_mu = sum_c (mu_c - y_c)^2 - sum_c v^_c,      q_out = sum_c (out_c - y_c)^2 + sum_c (2 W_cc - 1) v^_c.
    A pixel is valid iff all its inputs are finite and every pivot is > 0; a degenerate pixel is counted and left out of everything
    else.  Only the pixels margin <= i < e1 - margin, margin <= j < e2 - margin of a sample's extent ext[b] = (e1, e2) (None: the whole
    tensor; clamped to it) take part.  There is no 1e-6 regulariser: the heads place theirs differently, far below the estimator's
    resolution wherever n_c >> 1e-6.
    -> {"stats": float64 [B,12]: N, degenerate, sum d2, sum logdet, sum |mu - y|^2, sum |out - y|^2, sum sum_c v^_c,
    sum sum_c (2 W_cc - 1) v^_c, sum q_mu^2, sum q_out^2, sum tr W, the (valid pixel, channel) pairs with y_c <= 0 or y_c >= 1 (clipped
    samples, where the noise is not zero-mean: reported, not removed -- removing them would select)} and the values `risk_values`
    derives, float64 [B] each.  maps=True adds "q_mu" and "q_out" [B,H,W], NaN outside the region and at degenerate pixels."""
    if noisy.dim() != 4 or noisy.shape[1] not in (1, 3):
        raise ValueError("calculate_risk: noisy must be BCHW with C in {1, 3}, got %s" % (tuple(noisy.shape),))
    B, C, H, W = noisy.shape
    for name, t in (("mu", mu), ("out", out), ("noise_var", noise_var), ("var_hat", var_hat)):
        if tuple(t.shape) != (B, C, H, W):
            raise ValueError("calculate_risk: %s must be %s, got %s" % (name, (B, C, H, W), tuple(t.shape)))
    if tuple(cov_x.shape) != (B, C * (C + 1) // 2, H, W):
        raise ValueError("calculate_risk: cov_x must be %s, got %s" % ((B, C * (C + 1) // 2, H, W), tuple(cov_x.shape)))
    if int(margin) < 0:
        raise ValueError("calculate_risk: margin must be at least 0, got %s" % (margin,))
    margin = int(margin)
    dev = noisy.device
    y, m, s, o, n, v = (t.to(torch.float64) for t in (noisy, mu, cov_x, out, noise_var, var_hat))
    fin = torch.ones((B, H, W), dtype=torch.bool, device=dev)
    for t in (y, m, s, o, n, v):
        fin = fin & torch.isfinite(t).all(1)
    if ext is None:
        e = torch.tensor([[H, W]] * B, dtype=torch.int64, device=dev)
    else:
        e = torch.as_tensor(ext, device=dev).to(torch.int64).reshape(B, 2)
    e1 = e[:, 0].clamp(0, H)[:, None, None]
    e2 = e[:, 1].clamp(0, W)[:, None, None]
    ii = torch.arange(H, device=dev)[None, :, None]
    jj = torch.arange(W, device=dev)[None, None, :]
    region = (ii >= margin) & (ii < e1 - margin) & (jj >= margin) & (jj < e2 - margin)
    d = y - m
    if C == 3:
        n0, n1, n2 = n[:, 0], n[:, 1], n[:, 2]
        t00, t01, t02, t11, t12, t22 = s[:, 0] + n0, s[:, 1], s[:, 2], s[:, 3] + n1, s[:, 4], s[:, 5] + n2
        p0 = t00
        l00 = torch.sqrt(p0)
        l10, l20 = t01 / l00, t02 / l00
        p1 = t11 - l10 * l10
        l11 = torch.sqrt(p1)
        l21 = (t12 - l20 * l10) / l11
        p2 = (t22 - l20 * l20) - l21 * l21
        l22 = torch.sqrt(p2)
        w0 = d[:, 0] / l00
        w1 = (d[:, 1] - l10 * w0) / l11
        w2 = ((d[:, 2] - l20 * w0) - l21 * w1) / l22
        d2 = (w0 * w0 + w1 * w1) + w2 * w2
        logdet = (torch.log(p0) + torch.log(p1)) + torch.log(p2)
        li00, li11, li22 = 1.0 / l00, 1.0 / l11, 1.0 / l22
        li10 = -(l10 * li00) / l11
        li21 = -(l21 * li11) / l22
        li20 = -(l20 * li00 + l21 * li10) / l22
        ti = ((li00 * li00 + li10 * li10) + li20 * li20, li11 * li11 + li21 * li21, li22 * li22)
        wcc = [1.0 - n[:, c] * ti[c] for c in range(3)]
        valid = fin & (p0 > 0) & (p1 > 0) & (p2 > 0)
    else:
        p0 = s[:, 0] + n[:, 0]
        d2 = (d[:, 0] * d[:, 0]) / p0
        logdet = torch.log(p0)
        wcc = [1.0 - n[:, 0] / p0]
        valid = fin & (p0 > 0)

    def over(f):                        # a per-pixel sum over the channels, left to right
        acc = f(0)
        for c in range(1, C):
            acc = acc + f(c)
        return acc
    em = over(lambda c: (m[:, c] - y[:, c]) * (m[:, c] - y[:, c]))
    eo = over(lambda c: (o[:, c] - y[:, c]) * (o[:, c] - y[:, c]))
    sv = over(lambda c: v[:, c])
    sw = over(lambda c: (2.0 * wcc[c] - 1.0) * v[:, c])
    trw = over(lambda c: wcc[c])
    q_mu, q_out = em - sv, eo + sw
    valid = valid & region
    clipped = over(lambda c: ((y[:, c] <= 0.0) | (y[:, c] >= 1.0)).to(torch.float64))
    zero = torch.zeros((), dtype=torch.float64, device=dev)

    def total(t):
        return torch.where(valid, t, zero).reshape(B, -1).sum(1)
    cols = [valid.reshape(B, -1).sum(1).to(torch.float64), (region & ~valid).reshape(B, -1).sum(1).to(torch.float64), total(d2),
            total(logdet), total(em), total(eo), total(sv), total(sw), total(q_mu * q_mu), total(q_out * q_out), total(trw), total(clipped)]
    stats = torch.stack(cols, 1)
    res = {"stats": stats}
    res.update(risk_values(stats, C))
    if maps:
        nan = torch.full_like(q_mu, float("nan"))
        res["q_mu"] = torch.where(valid, q_mu, nan)
        res["q_out"] = torch.where(valid, q_out, nan)
    return res


# ---- blind noise-level estimation (SSDN_OP_NOISE_EST, csrc/noise_est.hip) -------------------------------------------------------
NOISE_EST_CLASSES, NOISE_EST_BINS, NOISE_EST_NMIN = 8, 1024, 256
NOISE_EST_C = 6 * 0.6744897501960817             # |r| has standard deviation 6 sigma; the median of |N(0, 1)| is 0.6744...
NOISE_EST_SIGMA_FLOOR, NOISE_EST_LAMBDA_CAP = 0.5, 260100.0


def _grouped_median(q: Tensor) -> Tensor:
    """Grouped medians of the histograms q [..., 1024] (int64) -> float64 [...]: half = N/2, k* the smallest bin with cum(k*) >= half,
    med = lo + (hi - lo)(half - cum(k* - 1)) / q[k*] on the bin's edges lo = max(k* - 0.5, 0), hi = k* + 0.5; NaN for N = 0 or for
    k* = 1023, the clamp bin."""
    cum = q.cumsum(-1)
    N = cum[..., -1:]
    k = ((2 * cum >= N).to(torch.int64).cumsum(-1) == 0).sum(-1, keepdim=True).clamp(max=q.shape[-1] - 1)    # the first bin that reaches half
    qk = q.gather(-1, k)
    below = cum.gather(-1, k) - qk
    half = N.to(torch.float64) / 2.0
    kf = k.to(torch.float64)
    lo, hi = torch.clamp(kf - 0.5, min=0.0), kf + 0.5
    med = lo + ((hi - lo) * (half - below.to(torch.float64))) / qk.to(torch.float64)
    nan = torch.full_like(med, float("nan"))
    return torch.where((N > 0) & (k < q.shape[-1] - 1), med, nan)[..., 0]


def noise_estimates(hist: Tensor, ssum: Tensor) -> Dict:
    """The estimates of `estimate_noise` from one image's integer table (hist int64 [8,1024], ssum int64 [8]), float64 on their device."""
    f64 = torch.float64
    hist, ssum = hist.to(torch.int64), ssum.to(torch.int64)
    nan = torch.full((), float("nan"), dtype=f64, device=hist.device)
    ng = hist.sum(1)
    n = int(ng.sum())
    sigma = nan
    if n >= NOISE_EST_NMIN:
        sigma = _grouped_median(hist.sum(0)) / NOISE_EST_C
        sigma = torch.where(sigma < NOISE_EST_SIGMA_FLOOR, torch.full_like(sigma, NOISE_EST_SIGMA_FLOOR), sigma)      # (NaN stays NaN)
    keep = ng >= NOISE_EST_NMIN
    nanv = torch.full((NOISE_EST_CLASSES,), float("nan"), dtype=f64, device=hist.device)
    sg = torch.where(keep, _grouped_median(hist) / NOISE_EST_C, nanv)
    mg = torch.where(keep, ssum.to(f64) / (9.0 * ng.to(f64)), nanv)
    num = den = torch.zeros((), dtype=f64, device=hist.device)
    used = 0
    for g in range(NOISE_EST_CLASSES):              # a least-squares fit of sigma_g^2 = 255 m_g / lambda through the origin, g ascending
        if bool(keep[g]):
            nm = ng[g].to(f64) * mg[g]
            num = num + nm * mg[g]
            den = den + nm * (sg[g] * sg[g])
            used += 1
    lam = nan
    if used:
        cap = torch.full((), NOISE_EST_LAMBDA_CAP, dtype=f64, device=hist.device)
        lam = cap if float(den) == 0.0 else (255.0 * num) / den
        lam = torch.where(lam > cap, cap, lam)                                                                         # (NaN stays NaN)
    return {"sigma": float(sigma), "lambda": float(lam), "n": n, "classes_used": used, "nlf_sigma": sg.cpu(), "nlf_mean": mg.cpu()}


def estimate_noise(image_u8, hist: bool = False) -> Dict:
    """A blind estimate of the noise level of one image -- the specification SSDN_OP_NOISE_EST (csrc/noise_est.hip) is held to: exact
    integers for the table, float64 after it, on the image's device.  image_u8: an upright uint8 array or tensor [h, w] or [h, w, C].
    Per 3x3 window, i.e. per (y, x, c) with 1 <= y <= h-2 and 1 <= x <= w-2 (the channels pool into one table):
        r = sum K p with K = [[1,-2,1],[-2,4,-2],[1,-2,1]] (Immerkaer 1996: for i.i.d. noise of variance v, Var r = 36 v, and locally
        planar image content cancels), S = sum p; the window is valid iff all nine bytes lie in [1, 254] (0 and 255 may be clipped
        values); intensity class g = (S // 9) >> 5; bin k = min(|r|, 1023).
    hist[g][k] counts the valid windows, ssum[g] adds their S; n_g and n are the counts per class and in all.  With the grouped median
    med(.) of a histogram (NaN in the clamp bin), c = 6 * 0.6744897501960817 and NMIN = 256:
        sigma  = max(med(sum_g hist[g]) / c, 0.5), in byte units (the 25 of gauss25); NaN if n < NMIN
        for every class with n_g >= NMIN: nlf_sigma[g] = med(hist[g]) / c, nlf_mean[g] = ssum[g] / (9 n_g); other classes NaN, left out
        lambda = min(255 sum n_g m_g^2 / sum n_g m_g sigma_g^2, 260100) over the classes kept (the Poisson head's Var = mu / lambda, in
                 byte units 255 m / lambda); a zero denominator gives the cap; NaN if no class is kept.
    The floors give a noise-free picture a finite positive parameter.  Biases measured on synthetic pictures: DESIGN.md section 3.17.
    -> {"sigma", "lambda": floats, "n", "classes_used": ints, "nlf_sigma", "nlf_mean": float64 [8]}; hist=True adds "hist" int64
    [8,1024] and "ssum" int64 [8]."""
    import numpy as np
    t = image_u8
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t))
    if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.dim() not in (2, 3):
        raise ValueError("estimate_noise: a uint8 array or tensor [h, w] or [h, w, C]")
    p = (t.unsqueeze(-1) if t.dim() == 2 else t).to(torch.int64)
    h, w, C = p.shape
    table = torch.zeros((NOISE_EST_CLASSES * NOISE_EST_BINS,), dtype=torch.int64, device=p.device)
    ssum = torch.zeros((NOISE_EST_CLASSES,), dtype=torch.int64, device=p.device)
    if h >= 3 and w >= 3:
        K = ((1, -2, 1), (-2, 4, -2), (1, -2, 1))
        r = torch.zeros((h - 2, w - 2, C), dtype=torch.int64, device=p.device)
        S = torch.zeros_like(r)
        valid = torch.ones_like(r, dtype=torch.bool)
        for dy in range(3):
            for dx in range(3):
                v = p[dy:h - 2 + dy, dx:w - 2 + dx]
                r += K[dy][dx] * v
                S += v
                valid &= (v >= 1) & (v <= 254)
        g = torch.div(S, 9, rounding_mode="floor") >> 5
        k = r.abs().clamp(max=NOISE_EST_BINS - 1)
        one = valid.to(torch.int64).reshape(-1)
        table.scatter_add_(0, (g * NOISE_EST_BINS + k).reshape(-1), one)
        ssum.scatter_add_(0, g.reshape(-1), S.reshape(-1) * one)
    table = table.view(NOISE_EST_CLASSES, NOISE_EST_BINS)
    res = noise_estimates(table, ssum)
    if hist:
        res["hist"], res["ssum"] = table, ssum
    return res


# ---- image I/O helpers of the trainer / evaluator (utils/data.py:69-125) ------------------------------------------------------
def tensor2image(img: Tensor):
    """CHW float tensor in [0,1] -> PIL image.  The dataset classes hand out tensors with H and W SWAPPED (PIL data
    labelled "CWH" and permuted, datasets/hdf5.py:62-72, folder.py:83-84 -- reproduced in ssdn.datasets), and this function
    swaps them back on the way out (utils/data.py:80), so saved PNGs are upright.  A BCHW batch becomes a horizontal strip."""
    import numpy as np
    from PIL import Image
    img = img.detach().cpu().float()
    if img.dim() == 4:
        img = torch.cat(list(img), dim=1)           # stack along the (swapped) first spatial axis = image x axis
    a = np.clip(img.numpy(), 0, 1).transpose(2, 1, 0)         # C, W', H' -> H', W', C
    if a.shape[-1] == 3:
        return Image.fromarray(np.uint8(a * 255), mode="RGB")
    if a.shape[-1] == 1:
        return Image.fromarray(np.uint8(a[..., 0] * 255), mode="L")
    raise NotImplementedError("Cannot convert image with {} channels to PIL image.".format(a.shape[-1]))


def save_tensor_image(img: Tensor, path: str):
    tensor2image(img).save(path)


def set_color_channels(img, channels: int):
    """PIL image -> 1 (weighted RGB->L) or 3 (replicated) channels (utils/data.py:114-125)."""
    cur = len(img.getbands())
    if cur != channels:
        if channels == 1:
            return img.convert("L")
        if channels == 3:
            return img.convert("RGB")
    return img


PIL_MODES_16 = ("I;16", "I;16L", "I;16B", "I;16N")


def image_bits(mode: str) -> int:
    """16 for the PIL modes `load_image` returns as uint16 (mode "I" included: a 16-bit file some decoders widen), else 8"""
    return 16 if mode in PIL_MODES_16 or mode == "I" else 8


def load_image(path: str, channels: int):
    """An image file as the array `Denoiser.denoise` takes: uint8 [h, w, C] through `set_color_channels` for every file that is 8-bit, uint16
    [h, w, 1] in host byte order for a 16-bit grey file (PIL modes I;16, I;16L, I;16B, I;16N, and I where every value lies in [0, 65535]:
    ValueError otherwise).  `img.convert` clips such a file at 255, so it never goes that way; PIL cannot deliver 16-bit RGB, so a 16-bit
    file with channels == 3 is refused -- arrays are the route for that."""
    import numpy as np
    from PIL import Image
    with open(path, "rb") as f:
        img = Image.open(f)
        img.load()
    if image_bits(img.mode) == 16:
        if channels != 1:
            raise ValueError("%s: 16-bit files are single-channel: use a model trained with --mono" % path)
        a = np.asarray(img)
        if img.mode == "I" and a.size and (a.min() < 0 or a.max() > 65535):
            raise ValueError("%s: a 32-bit integer image with values outside [0, 65535] is not a 16-bit image" % path)
        return np.ascontiguousarray(a.astype(np.uint16)).reshape(a.shape[0], a.shape[1], 1)
    a = np.asarray(set_color_channels(img, channels), dtype=np.uint8)
    return np.ascontiguousarray(a).reshape(a.shape[0], a.shape[1], -1)


def save_image16(array, path: str):
    """uint16 [h, w] or [h, w, 1] (array or tensor) -> a 16-bit grey image file (PIL mode I;16; exact through PNG and TIFF)"""
    import numpy as np
    from PIL import Image
    a = array.numpy() if torch.is_tensor(array) else np.asarray(array)
    if a.dtype != np.uint16 or not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 1)):
        raise ValueError("save_image16: a uint16 array [h, w] or [h, w, 1] is needed, got %s %s" % (a.dtype, tuple(a.shape)))
    Image.fromarray(np.ascontiguousarray(a.reshape(a.shape[0], a.shape[1]))).save(path)
