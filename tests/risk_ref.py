"""A plain numpy model of SSDN_OP_RISK / ssdn.utils.calculate_risk, written from the definition (include/ssdn_hip.h) with numpy.linalg and
nothing of the package: Sigma_x = U U^T, the sigma rule, a float32 softplus for the learnt estimate, T^-1 and log det T from
numpy.linalg.inv / slogdet.  Also the input builder of the tests, which itself asserts what makes tight comparisons legitimate, and the
toy blind function of the identity test."""
import numpy as np

NSTATS = 12
FLOAT_SUMS = (2, 3, 4, 5, 6, 7, 8, 9, 10)
COUNTS = (0, 1, 11)
TRI = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
STYLE = {"gauss": 0, "poisson": 1}
MODE = {"known": 0, "const": 1, "var": 2}


def softplus_m4_f32(raw):
    """torch.nn.Softplus(beta=1, threshold=20) of (raw - 4), + 1e-3, every step in float32"""
    x = np.float32(raw) - np.float32(4.0)
    if x > np.float32(20.0):
        return np.float32(x + np.float32(1e-3))
    return np.float32(np.log1p(np.exp(x, dtype=np.float32), dtype=np.float32) + np.float32(1e-3))


def sigma_x(net_out, C, diag):
    """net_out [B,Cout,H,W] float32 -> Sigma_x [B,H,W,C,C] float64: U U^T with U = [[a0,a1,a2],[0,a3,a4],[0,0,a5]], or diag(a_c^2)"""
    A = net_out[:, C:].astype(np.float64)
    B, _, H, W = net_out.shape
    U = np.zeros((B, H, W, C, C))
    if C == 1 or diag:
        for c in range(C):
            U[..., c, c] = A[:, c]
    else:
        for k, (i, j) in enumerate(TRI):
            U[..., i, j] = A[:, k]
    return U @ np.swapaxes(U, -1, -2)


def noise_terms(net_out, noisy, noise_param, est_raw, C, style, mode):
    """-> (n [B,C,H,W], v_hat [B,C,H,W]) float64 by the definition's sigma rule"""
    B = net_out.shape[0]
    mu32 = net_out[:, :C]
    n = np.zeros(mu32.shape)
    v = np.zeros(mu32.shape)
    for b in range(B):
        est = np.float64(softplus_m4_f32(est_raw[b if mode == 2 else 0])) if mode != 0 else None
        if style == 0:
            sig = np.float64(np.maximum(np.float32(noise_param[b]), np.float32(1e-3))) if mode == 0 else est
            n[b] = sig * sig
            v[b] = n[b]
        else:
            f = 1.0 / np.float64(np.float32(noise_param[b])) if mode == 0 else est
            n[b] = np.maximum(mu32[b], np.float32(1e-3)).astype(np.float64) * f
            v[b] = noisy[b].astype(np.float64) * f
    return n, v


def definition_inputs(net_out, noisy, noise_param, est_raw, C, style, mode, diag):
    """what ssdn.utils.calculate_risk takes besides noisy and out: mu, cov_x (upper triangle), noise_var, var_hat, float64"""
    S = sigma_x(net_out, C, diag)
    cov = np.stack([S[..., i, j] for i, j in (TRI if C == 3 else ((0, 0),))], 1)
    n, v = noise_terms(net_out, noisy, noise_param, est_raw, C, style, mode)
    return net_out[:, :C].astype(np.float64), cov, n, v


def per_pixel(noisy, mu, S, out, n, v):
    """the definition's per-pixel values through numpy.linalg: noisy, mu, out, n, v [B,C,H,W]; S [B,H,W,C,C], float64 ->
    dict of [B,H,W] arrays (valid: bool) -- NaN wherever the pixel is degenerate"""
    B, C, H, W = noisy.shape
    y, m, o = (np.moveaxis(t.astype(np.float64), 1, -1) for t in (noisy, mu, out))
    nn, vv = np.moveaxis(n, 1, -1), np.moveaxis(v, 1, -1)
    T = S + nn[..., :, None] * np.eye(C)
    fin = np.isfinite(y).all(-1) & np.isfinite(m).all(-1) & np.isfinite(o).all(-1) & np.isfinite(nn).all(-1) & np.isfinite(vv).all(-1)
    fin &= np.isfinite(S).all((-1, -2))
    Ts = np.where(fin[..., None, None], T, np.eye(C))
    pd = fin & (np.linalg.eigvalsh(Ts).min(-1) > 0)
    Ts = np.where(pd[..., None, None], Ts, np.eye(C))
    Ti = np.linalg.inv(Ts)
    sign, logdet = np.linalg.slogdet(Ts)
    d = (y - m)[..., None]
    d2 = (np.swapaxes(d, -1, -2) @ Ti @ d)[..., 0, 0]
    Wm = np.where(pd[..., None, None], S, 0.0) @ Ti
    wcc = np.stack([Wm[..., c, c] for c in range(C)], -1)
    em, eo = ((m - y) ** 2).sum(-1), ((o - y) ** 2).sum(-1)
    sv, sw = vv.sum(-1), ((2 * wcc - 1) * vv).sum(-1)
    asv, asw = np.abs(vv).sum(-1), np.abs((2 * wcc - 1) * vv).sum(-1)
    res = dict(d2=d2, logdet=logdet, em=em, eo=eo, sv=sv, sw=sw, q_mu=em - sv, q_out=eo + sw, trw=wcc.sum(-1), asv=asv, asw=asw,
               clipped=((y <= 0) | (y >= 1)).sum(-1).astype(np.float64), cond=np.linalg.cond(Ts))
    res = {k: np.where(pd, t, np.nan) for k, t in res.items()}
    res["valid"] = pd
    return res


def region_mask(B, H, W, ext, margin):
    mask = np.zeros((B, H, W), dtype=bool)
    for b in range(B):
        e1, e2 = (H, W) if ext is None else (min(max(int(ext[b][0]), 0), H), min(max(int(ext[b][1]), 0), W))
        if e1 - margin > margin and e2 - margin > margin:
            mask[b, margin:e1 - margin, margin:e2 - margin] = True
    return mask


def stats_from(px, mask):
    """-> (stats [B,12], scale [B,12], wide [B,12]): the twelve statistics over each sample's region, and per floating-point sum the sum
    of its terms' absolute values (what a comparison of two summation orders is relative to).  `scale` takes a pixel's value as the
    term; `wide` goes down to the terms a pixel's value is itself made of, which matters where they cancel: sum_c |v^_c| and
    sum_c |(2 W_cc - 1) v^_c| for statistics 6 and 7, and for the squares q^2 = (e - s)^2 of statistics 8 and 9 (e + |s|)^2 -- a relative
    perturbation delta of the noise estimate moves s by delta |s| and q^2 by 2 |q| delta |s| <= 2 delta (e + |s|)^2, whatever q is."""
    B = mask.shape[0]
    stats, scale, wide = np.zeros((B, NSTATS)), np.zeros((B, NSTATS)), np.zeros((B, NSTATS))
    wide_terms = {6: px["asv"], 7: px["asw"], 8: (px["em"] + px["asv"]) ** 2, 9: (px["eo"] + px["asw"]) ** 2}
    terms = {2: px["d2"], 3: px["logdet"], 4: px["em"], 5: px["eo"], 6: px["sv"], 7: px["sw"], 8: px["q_mu"] ** 2, 9: px["q_out"] ** 2,
             10: px["trw"], 11: px["clipped"]}
    for b in range(B):
        ok = mask[b] & px["valid"][b]
        stats[b, 0], stats[b, 1] = ok.sum(), (mask[b] & ~px["valid"][b]).sum()
        for k, t in terms.items():
            stats[b, k] = t[b][ok].sum()
            scale[b, k] = np.abs(t[b][ok]).sum()
            wide[b, k] = wide_terms[k][b][ok].sum() if k in wide_terms else scale[b, k]
    return stats, scale, wide


def risk_model(net_out, noisy, pme, noise_param, est_raw, style, mode, diag, ext=None, margin=0):
    """the op as the header defines it -> (stats [B,12], scale [B,12], per-pixel dict); the per-pixel dict also carries "wide", the
    scale of stats_from that goes down to the terms of a pixel's value"""
    B, C, H, W = noisy.shape
    mu, _, n, v = definition_inputs(net_out, noisy, noise_param, est_raw, C, style, mode, diag)
    with np.errstate(all="ignore"):
        px = per_pixel(noisy.astype(np.float64), mu, sigma_x(net_out, C, diag), pme.astype(np.float64), n, v)
    stats, scale, wide = stats_from(px, region_mask(B, H, W, ext, margin))
    px["wide"] = wide
    return stats, scale, px


def make_inputs(B, C, H, W, style="gauss", mode="known", diag=False, seed=0):
    """Well-conditioned inputs of the op: -> dict(net_out [B,Cout,H,W], noisy, pme [B,C,H,W], noise_param [B], est_raw [B]) float32.
    Asserted here: the entries of Sigma_x lie between 1e-4 and 1e-2 (diag: its diagonal), cond(T) <= 1e4, no pixel is degenerate and
    no y_c is exactly 0 or 1."""
    rng = np.random.default_rng(1000 * seed + 7 * C + H)
    st, mo = STYLE[style], MODE[mode]
    NA = C if (diag or C == 1) else 6
    mu = rng.uniform(0.1, 0.9, (B, C, H, W))
    A = np.zeros((B, NA, H, W))
    for k in range(NA):
        on_diag = NA != 6 or TRI[k][0] == TRI[k][1]
        A[:, k] = rng.uniform(0.03, 0.06, (B, H, W)) if on_diag else rng.uniform(0.01, 0.03, (B, H, W))
    net_out = np.concatenate([mu, A], 1).astype(np.float32)
    noisy = (mu + rng.normal(0, 0.1, mu.shape)).astype(np.float32)
    noisy[(noisy == 0) | (noisy == 1)] = np.float32(0.5)
    pme = (0.6 * mu + 0.4 * noisy + rng.normal(0, 0.01, mu.shape)).astype(np.float32)
    if st == 0:
        noise_param = rng.uniform(20, 30, B).astype(np.float32) / np.float32(255)
        est_raw = rng.uniform(1.6, 1.9, B).astype(np.float32)         # softplus(raw - 4) + 1e-3: sigma ~ 0.09 .. 0.12
    else:
        noise_param = rng.uniform(25, 40, B).astype(np.float32)
        est_raw = rng.uniform(0.6, 0.9, B).astype(np.float32)         # 1 / lambda ~ 0.033 .. 0.045
    S = sigma_x(net_out, C, diag)
    ent = np.stack([S[..., c, c] for c in range(C)]) if (diag or C == 1) else np.stack([S[..., i, j] for i, j in TRI])
    assert 1e-4 <= ent.min() and ent.max() <= 1e-2, (ent.min(), ent.max())
    _, _, px = risk_model(net_out, noisy, pme, noise_param, est_raw, st, mo, int(diag))
    assert px["valid"].all() and np.nanmax(px["cond"]) <= 1e4 and not ((noisy == 0) | (noisy == 1)).any()
    return dict(net_out=net_out, noisy=noisy, pme=pme, noise_param=noise_param, est_raw=est_raw, style=st, mode=mo, diag=int(diag))


# ---- the identity: a toy blind function -------------------------------------------------------------------------------------------
def toy_clean(C, H=48, W=64):
    """0.5 + 0.35 sin(x/37) cos(y/53) + 0.1 sin((x+y)/11), rolled by 7c rows per channel, clipped to [0.05, 0.95]"""
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    base = 0.5 + 0.35 * np.sin(xx / 37) * np.cos(yy / 53) + 0.1 * np.sin((xx + yy) / 11)
    return np.clip(np.stack([np.roll(base, 7 * c, axis=0) for c in range(C)]), 0.05, 0.95)


def toy_noisy(clean, style, seed):
    """gauss sigma = 25/255, or true Poisson counts rng.poisson(30 x) / 30 -> (noisy, n_c of the model, f)"""
    rng = np.random.default_rng(seed)
    if style == "gauss":
        return clean + rng.normal(0, 25 / 255, clean.shape)
    return rng.poisson(30 * clean) / 30.0


def toy_blind(noisy, style):
    """A function of each pixel's eight reflect-padded neighbours only -> (mu [C,H,W], S [H,W,C,C], n [C,H,W], v_hat [C,H,W],
    out [C,H,W], W_cc [C,H,W]):  nb = the neighbours' mean, mu = 0.8 nb + 0.1 mean_c(nb) + 0.03, Sigma_x = A A^T with A upper
    triangular, A_ii = 0.05 + 0.1 |nb_(2i mod C) - 1/2|, A_ij = 0.02 (nb_i - nb_j), out = mu + Sigma_x T^-1 (y - mu)."""
    C, H, W = noisy.shape
    p = np.pad(noisy, ((0, 0), (1, 1), (1, 1)), mode="reflect")
    nb = sum(p[:, 1 + di:1 + di + H, 1 + dj:1 + dj + W] for di in (-1, 0, 1) for dj in (-1, 0, 1) if (di, dj) != (0, 0)) / 8.0
    mu = 0.8 * nb + 0.1 * nb.mean(0, keepdims=True) + 0.03
    A = np.zeros((H, W, C, C))
    for i in range(C):
        A[..., i, i] = 0.05 + 0.1 * np.abs(nb[(2 * i) % C] - 0.5)
        for j in range(i + 1, C):
            A[..., i, j] = 0.02 * (nb[i] - nb[j])
    S = A @ np.swapaxes(A, -1, -2)
    if style == "gauss":
        n = np.full(noisy.shape, (25 / 255) ** 2)
        v = n.copy()
    else:
        n = np.maximum(mu, 1e-3) / 30.0
        v = noisy / 30.0
    T = S + np.moveaxis(n, 0, -1)[..., :, None] * np.eye(C)
    Wm = S @ np.linalg.inv(T)
    d = np.moveaxis(noisy - mu, 0, -1)[..., None]
    out = mu + np.moveaxis((Wm @ d)[..., 0], -1, 0)
    wcc = np.stack([Wm[..., c, c] for c in range(C)])
    return mu, S, n, v, out, wcc
