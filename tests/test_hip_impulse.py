"""GPU: the impulse noise model -- SSDN_OP_NOISE style 2 (k_noise_impulse), k_head_impulse and
k_head_vjp_impulse teacher-forced against the float64 mirror (tests/test_impulse_cpu.py, itself pinned to autograd of the paper's form),
the Denoiser end to end (x.grad, mean(LOSS) bit-identity, a 3-step Adam trajectory next to a CPU loop, evaluation at a non-training
size, a `.wt` round trip, a plan blob through the C ABI alone, gradient accumulation) and the trainer's command line.

The gauss / poisson arms of SSDN_OP_NOISE are compared with CHECKSUMS WRITTEN DOWN from a library built at the parent commit, run on an
MI355X (PARENT_NOISE_SUMS): the sum of the output's float bits and coordinates, as int64, of two fixed launches."""
import csv
import glob
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import restate as R
from test_impulse_cpu import impulse_cfg, impulse_forward_paper, impulse_head, impulse_inputs
from test_hip_denoiser import _cat_state, _flat_grad_of, _flat_of
from test_hip_denoiser_autograd import DEV, P, _cos_rel
from head_ops import head_op, head_vjp_op
from test_hip_noise import _run as noise_run

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STYLE_IMPULSE = 2


def close(a, b, rtol, atol, what=""):
    b = b.detach().cpu().double().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    a = a.detach().cpu().double().numpy().reshape(b.shape)
    err = np.abs(a - b)
    print("%s: max abs err %.3e (max |want| %.3e)" % (what, float(err.max()) if err.size else 0.0, float(np.abs(b).max()) if b.size else 0.0))
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol, err_msg=what)


# ---- 1. SSDN_OP_NOISE, style 2 ------------------------------------------------------------------------------------------------------------------
def _u8(shape, seed):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _masks(o, key="noisy"):
    ch = o[key] != o["clean"]
    return ch.any(1), ch.all(1)


def test_noise_op_impulse_statistics_and_determinism():
    u8 = _u8((32, 3, 64, 64), 1)
    alpha = 0.3
    o = noise_run(u8, STYLE_IMPULSE, True, alpha, alpha, seed=7, offset=3, ref=True)
    assert torch.equal(o["clean"], u8.float() / 255.0)
    assert float((o["param"] - np.float32(alpha)).abs().max()) == 0.0 and float((o["param_ref"] - np.float32(alpha)).abs().max()) == 0.0
    masks = {}
    for key in ("noisy", "ref"):
        y = o[key]
        any_c, all_c = _masks(o, key)
        n = any_c.numel()
        # an fp32 coincidence of (k + 1/2) / 2^24 with j / 255 in one channel is possible, a systematic one is not
        assert int((any_c & ~all_c).sum()) <= 1e-5 * int(any_c.sum()), key
        assert torch.equal(y[~any_c[:, None].expand_as(y)], o["clean"][~any_c[:, None].expand_as(y)])       # untouched pixels: exactly u8 / 255
        frac = float(any_c.float().mean())
        assert abs(frac - alpha) <= 5 * math.sqrt(alpha * (1 - alpha) / n), (key, frac)
        vals = y[any_c[:, None].expand_as(y)].double()
        assert abs(float(vals.mean()) - 0.5) <= 5 * math.sqrt(1 / 12 / vals.numel()), key
        assert abs(float(vals.var()) - 1 / 12) <= 5 * math.sqrt(1 / 180 / vals.numel()), key
        assert 0.0 < float(vals.min()) and float(vals.max()) < 1.0
        chans = y.permute(1, 0, 2, 3)[:, any_c].double()                 # the three colours of a replaced pixel are independent draws
        assert abs(float(torch.corrcoef(chans)[0, 1])) <= 5 / math.sqrt(chans.shape[1])
        masks[key] = any_c
    # the second realisation is independent of the first
    a, b = masks["noisy"].flatten().double(), masks["ref"].flatten().double()
    assert abs(float(torch.corrcoef(torch.stack([a, b]))[0, 1])) <= 5 / math.sqrt(a.numel())
    # a pure function of (seed, offset)
    again = noise_run(u8, STYLE_IMPULSE, True, alpha, alpha, seed=7, offset=3, ref=True)
    assert torch.equal(again["noisy"], o["noisy"]) and torch.equal(again["ref"], o["ref"])
    other = noise_run(u8, STYLE_IMPULSE, True, alpha, alpha, seed=7, offset=4)
    c = _masks(other)[0].flatten().double()
    assert abs(float(torch.corrcoef(torch.stack([a, c]))[0, 1])) <= 5 / math.sqrt(a.numel())
    # `_nc` has nothing to clip
    assert torch.equal(noise_run(u8, STYLE_IMPULSE, False, alpha, alpha, seed=7, offset=3)["noisy"], o["noisy"])
    # mono
    m = noise_run(_u8((8, 1, 64, 64), 2), STYLE_IMPULSE, True, 0.5, 0.5, seed=9)
    fr = float((m["noisy"] != m["clean"]).float().mean())
    assert abs(fr - 0.5) <= 5 * math.sqrt(0.25 / m["noisy"].numel())


def test_noise_op_impulse_ranged_alpha_is_one_per_sample():
    u8 = _u8((32, 3, 64, 64), 3)
    o = noise_run(u8, STYLE_IMPULSE, True, 0.1, 0.6, seed=5, offset=1, ref=True)
    for key, mk in (("param", "noisy"), ("param_ref", "ref")):
        par = o[key]
        assert float(par.min()) >= 0.1 and float(par.max()) < 0.6
        assert bool((par == par[:, :1]).all()) and len(torch.unique(par[:, 0])) == 32              # all C entries hold the sample's alpha
        frac = _masks(o, mk)[0].float().mean(dim=(1, 2))
        tol = 5 * (par[:, 0] * (1 - par[:, 0]) / 4096).sqrt()
        assert bool(((frac - par[:, 0]).abs() <= tol).all()), key
    assert not torch.equal(o["param"], o["param_ref"])


def test_noise_op_impulse_noise2void():
    u8 = _u8((8, 3, 64, 64), 4)
    plain = noise_run(u8, STYLE_IMPULSE, True, 0.4, 0.4, seed=11, offset=2, ref=True)
    o = noise_run(u8, STYLE_IMPULSE, True, 0.4, 0.4, seed=11, offset=2, ref=True, n2v=True)
    assert torch.equal(o["ref"], plain["ref"]) and torch.equal(o["clean"], plain["clean"])
    co = o["coords"]
    assert tuple(co.shape) == (8, 64, 2) and int(co.min()) >= 0 and int(co.max()) < 64
    sel = torch.zeros((8, 64, 64), dtype=torch.bool)
    for b in range(8):
        assert len({(int(x) // 8, int(y) // 8) for x, y in co[b].tolist()}) == 64                   # one pixel per 8 x 8 box
        for x, y in co[b].tolist():
            sel[b, y, x] = True
            cand_x = [v % 64 for v in range(min(x - 2, 0), min(x + 2, 63) + 1)]
            cand_y = [v % 64 for v in range(min(y - 2, 0), min(y + 2, 63) + 1)]
            src = (plain["noisy"][b][:, cand_y][:, :, cand_x] == o["noisy"][b][:, y, x].view(3, 1, 1)).all(0)
            assert bool(src.any()), (b, x, y)                          # the un-manipulated noisy value of a pixel inside the window
    keep = ~sel[:, None].expand_as(o["noisy"])
    assert torch.equal(o["noisy"][keep], plain["noisy"][keep])


def test_noise_op_impulse_rejects_bad_arguments():
    import ctypes as C
    from ssdn.hip import lib as L
    lib = L.load()
    a = L.NoiseArgs()
    rec = (L.OpRec * 1)()
    rec[0].type, rec[0].args = L.OP["noise"], C.cast(C.pointer(a), C.c_void_p)
    buf = (C.c_float * 64)()
    a.clean_u8, a.noisy32 = C.cast(buf, C.c_void_p), C.cast(buf, C.c_void_p)
    a.B, a.C, a.H, a.W, a.style = 1, 1, 2, 2, 2
    a.p_lo, a.p_hi = 0.5, 1.5
    assert lib.ssdn_run_ops(rec, 1, None) != 0 and b"alpha" in lib.ssdn_last_error()
    a.p_lo, a.p_hi = -0.1, 0.5
    assert lib.ssdn_run_ops(rec, 1, None) != 0 and b"alpha" in lib.ssdn_last_error()
    a.p_lo, a.p_hi, a.C = 0.5, 0.5, 4
    assert lib.ssdn_run_ops(rec, 1, None) != 0 and b"channels" in lib.ssdn_last_error()
    a.style, a.C, a.p_lo, a.p_hi = 1, 1, 0.0, 0.0                       # the p_lo > 0 rule stays Poisson's
    assert lib.ssdn_run_ops(rec, 1, None) != 0 and b"lambda" in lib.ssdn_last_error()


# sum of the float bits (as int64) of noisy32 + ref32 of the two launches below, from a library built at the parent commit
PARENT_NOISE_SUMS = {"gauss25": 198858981125822, "poisson30": 206991052103710}


def _noise_sum(style):
    u8 = _u8((8, 3, 64, 64), 5)
    sty, p = (0, 25 / 255.0) if style == "gauss25" else (1, 30.0)
    o = noise_run(u8, sty, True, p, p, seed=13, offset=6, ref=True, n2v=True)
    return int(o["noisy"].view(torch.int32).long().sum() + o["ref"].view(torch.int32).long().sum() + o["coords"].sum())


@pytest.mark.parametrize("style", ["gauss25", "poisson30"])
def test_noise_op_other_styles_are_the_parents_bit_for_bit(style):
    got = _noise_sum(style)
    print("noise checksum %s: %d" % (style, got))
    assert PARENT_NOISE_SUMS[style] is not None and got == PARENT_NOISE_SUMS[style]


# ---- 2. / 3. the head ops, teacher-forced ---------------------------------------------------------------------------------------------------------
HEAD_CASES = [(C, mode, alpha) for C in (1, 3) for mode in ("known", "const", "var") for alpha in (0.05, 0.5)] + [(3, "const", 0.0965)]


def _est(raw, mode):
    return raw.mean(dim=(1, 2, 3)) if mode == "var" else raw


def _fp32_yardstick(net_out, noisy, npar, mode, est_raw, m64, w=None, gp=None, gm=None):
    """The mirror in fp32 torch against float64: what the number format alone costs on these inputs, per quantity (max abs error).  Where
    a diagonal entry of U is small (|a| of a few 1e-3 among entries of a few 1e-1) Sigma_x is ill-conditioned, the fp32 adjugate of
    Sigma_p = U U^T + 1e-6 I loses digits, and a pixel whose posterior weight is not saturated shows it."""
    m32 = impulse_head(net_out, noisy, npar, mode, est_raw, w, gp, gm, dtype=torch.float32)
    fig = {k: float((m32[k].double() - m64[k]).abs().max()) for k in ("loss", "pme", "g_net_out", "g_noisy")}
    # dL/dest_raw sums dL/dalpha over the pixels, the ill-conditioned ones included, and may nearly cancel (pme-only upstream terms)
    fig["g_est"] = float((m32["g_est"].double() - m64["g_est"]).abs().max()) if m64["g_est"] is not None else 0.0
    print("fp32 mirror vs float64, max abs error: " + ", ".join("%s %.2e (of max %.2e)" % (k, v, v / max(float(m64[k].abs().max()), 1e-300))
                                                                for k, v in fig.items() if m64[k] is not None))
    return fig


def _atol(start, fig):
    """the starting tolerance, widened to at most 4x the fp32 mirror's own error on the same inputs"""
    return max(start, 4 * fig)


@pytest.mark.parametrize("C,mode,alpha", HEAD_CASES)
def test_impulse_head_op_vs_float64(C, mode, alpha):
    net_out, noisy, npar, raw = impulse_inputs(C, mode, alpha)
    B, H = net_out.shape[0], net_out.shape[2]
    est_raw = _est(raw, mode) if raw is not None else None
    wm = torch.full((B,), 1.0 / B)
    m = impulse_head(net_out, noisy, npar, mode, est_raw, w=wm)
    fig = _fp32_yardstick(net_out, noisy, npar, mode, est_raw, m, w=wm)
    r = head_op(net_out, noisy, npar, "impulse", mode, est_raw)
    close(r["loss"], m["loss"], 2e-5, 1e-6, "loss")
    close(r["mu"], net_out[:, :C], 0, 0, "mu")
    close(r["pme"], m["pme"], 2e-5, _atol(5e-6, fig["pme"]), "pme")
    close(r["model_std"], m["model_std"], 2e-5, 1e-6, "model_std")
    close(r["noise_std"][:1] if mode == "const" else r["noise_std"], m["alpha"][:1 if mode == "const" else B], 2e-5, 1e-7, "alpha")
    g = m["g_net_out"]
    close(r["g_net_out"], g, 2e-4, _atol(1e-6 * float(g.abs().max()), fig["g_net_out"]), "g_net_out")
    if mode == "const":
        close(r["g_est"][:1], m["g_est"], 2e-4, _atol(1e-9, fig["g_est"]), "g_est")
    if mode == "var":
        want = (m["g_est"] / (H * H)).view(B, 1, 1, 1).expand(B, 1, H, H)
        close(r["g_sig"], want, 2e-4, _atol(1e-10, fig["g_est"] / (H * H)), "g_sigma_out")
    assert float(np.int32(r["gmax"][0].item()).view(np.float32)) == pytest.approx(float(r["g_net_out"].abs().max()), rel=1e-6)      # the sentinel: max |g| as written
    # another chunking: the per-pixel outputs do not change
    r2 = head_op(net_out, noisy, npar, "impulse", mode, est_raw, nchunks=1)
    assert torch.equal(r2["pme"], r["pme"]) and torch.equal(r2["g_net_out"], r["g_net_out"])


@pytest.mark.parametrize("C,mode,alpha", HEAD_CASES)
def test_impulse_head_vjp_op_vs_float64(C, mode, alpha):
    net_out, noisy, npar, raw = impulse_inputs(C, mode, alpha, seed=1)
    B, H = net_out.shape[0], net_out.shape[2]
    est_raw = _est(raw, mode) if raw is not None else None
    g = torch.Generator().manual_seed(17)
    w, gp, gm = torch.randn(B, generator=g), torch.randn(B, C, H, H, generator=g), torch.randn(B, C, H, H, generator=g)
    for terms in ((w, gp, gm), (w, None, None), (None, gp, None), (None, None, gm)):
        m = impulse_head(net_out, noisy, npar, mode, est_raw, *terms)
        fig = _fp32_yardstick(net_out, noisy, npar, mode, est_raw, m, *terms)
        r = head_vjp_op(net_out, noisy, npar, "impulse", mode, est_raw, *terms)
        og, ody = m["g_net_out"], m["g_noisy"]
        close(r["g_net_out"], og, 2e-4, _atol(2e-6 * float(og.abs().max()), fig["g_net_out"]), "g_net_out")
        close(r["g_noisy"], ody, 2e-4, _atol(4.1e-6 * float(ody.abs().max()) + 1e-30, fig["g_noisy"]), "g_noisy")
        if mode == "const":
            close(r["g_est"][:1], m["g_est"], 2e-4, _atol(1e-6 * float(m["g_est"].abs().max()) + 1e-12, fig["g_est"]), "g_est")
        if mode == "var":
            want = (m["g_est"] / (H * H)).view(B, 1, 1, 1).expand(B, 1, H, H)
            close(r["g_sig"], want, 2e-4, _atol(1e-6 * float(want.abs().max()) + 1e-12, fig["g_est"] / (H * H)), "g_sigma_out")
        assert float(np.int32(r["gmax"][0].item()).view(np.float32)) == pytest.approx(float(r["g_net_out"].abs().max()), rel=1e-6)
        # g_noisy = NULL: every other output unchanged, bit for bit
        r0 = head_vjp_op(net_out, noisy, npar, "impulse", mode, est_raw, *terms, g_noisy=False)
        assert torch.equal(r0["g_net_out"], r["g_net_out"]) and torch.equal(r0["partial"], r["partial"])
    # keep: a sample asking for exactly d mean(LOSS) keeps the forward's g_net_out and partials, bit for bit, and still writes g_noisy
    wm = torch.full((B,), 1.0 / B)
    f = head_op(net_out, noisy, npar, "impulse", mode, est_raw)
    r = head_vjp_op(net_out, noisy, npar, "impulse", mode, est_raw, wm, None, None, keep=1, g_init=f["g_net_out"], partial_init=f["partial"])
    assert torch.equal(r["g_net_out"], f["g_net_out"]) and torch.equal(r["partial"], f["partial"])
    mk = impulse_head(net_out, noisy, npar, mode, est_raw, wm)
    ody = mk["g_noisy"]
    close(r["g_noisy"], ody, 2e-4, _atol(4.1e-6 * float(ody.abs().max()), _fp32_yardstick(net_out, noisy, npar, mode, est_raw, mk, wm)["g_noisy"]),
          "g_noisy (keep)")
    # without keep the same request recomputes what the forward wrote
    r = head_vjp_op(net_out, noisy, npar, "impulse", mode, est_raw, wm, None, None)
    close(r["g_net_out"], f["g_net_out"], 1e-5, 1e-6 * float(f["g_net_out"].abs().max()), "VJP of mean(LOSS) vs the forward's gradient")


def test_impulse_head_refuses_diag():
    from ssdn.hip import lib as L
    from ssdn.hip.engine import OpList, current_stream
    t = torch.zeros(256, device=DEV)
    a = L.HeadArgs(P(t), P(t), P(t), None, 1, 3, 2, 2, STYLE_IMPULSE, 0, 1, None, None, None, None, P(t), P(t), 1, None, 1)
    with pytest.raises(L.SsdnHipError, match="impulse.*diag"):
        OpList([("head_ssdn", a)]).run(current_stream())
    v = L.HeadVjpArgs(P(t), P(t), P(t), None, 1, 3, 2, 2, STYLE_IMPULSE, 0, P(t), None, None, 0, 1, P(t), P(t), None, None, None, None)
    v.diag = 1
    with pytest.raises(L.SsdnHipError, match="impulse.*diag"):
        OpList([("head_vjp", v)]).run(current_stream())
    torch.cuda.synchronize()


# ---- 4. the Denoiser ------------------------------------------------------------------------------------------------------------------------------
ALPHA = 0.5


def impulse_denoiser(mode="known", ch=3, style="impulse50", seeded=True):
    """seeded: the main network from R.make_params(ch, ch + ch(ch+1)/2, True, seed=5), the sigma network (var) from seed 6, a learnt constant
    (const) at 1.7 -- the setting of tests/test_hip_denoiser_autograd.seeded_denoiser"""
    from ssdn.denoiser import Denoiser
    d = Denoiser(impulse_cfg(style, mode, ch), device="cuda:0")
    if seeded:
        d.get_model(Denoiser.MODEL, False).load_state_dict(R.reference_state_dict(R.make_params(ch, ch + ch * (ch + 1) // 2, True, seed=5)))
        if mode == "var":
            d.get_model(Denoiser.SIGMA_ESTIMATOR, False).load_state_dict(R.reference_state_dict(R.make_params(ch, 1, False, seed=6)))
        if mode == "const":
            with torch.no_grad():
                d.l_params[Denoiser.ESTIMATED_SIGMA].fill_(1.7)
        d.mark_dirty()
    d.train()
    return d


def impulse_batch(ch, B, Psz, seed=0, alpha=ALPHA, dev=True):
    from ssdn.datasets import NoisyDataset
    from ssdn.utils import noise
    MD = NoisyDataset.Metadata
    clean = (R.hash_tensor((B, ch, Psz, Psz), 161 + seed, 0, 1) * 255).round() / 255
    noisy, _ = noise.add_impulse(clean, alpha, generator=torch.Generator().manual_seed(100 + seed))
    meta = {MD.CLEAN: clean, MD.INPUT_NOISE_VALUES: torch.full((B, 1, 1, 1), alpha)}
    return [noisy.to(DEV) if dev else noisy, clean.to(DEV) if dev else clean, meta]


def reference_x_grad(d, mode, data, w, gp, gm):
    """x.grad through the model's NoiseNetwork autograd (+ the sigma network's, var) and the float64 paper-form head, whose noisy image
    is a leaf of its own"""
    from ssdn.denoiser import Denoiser
    import torch.nn.functional as F
    noisy = data[0]
    B = noisy.shape[0]
    xr = noisy.detach().clone().requires_grad_(True)
    out = d.get_model(Denoiser.MODEL, False)(xr)
    y64 = noisy.detach().cpu().double().requires_grad_(True)
    if mode == "known":
        alpha_b = torch.full((B,), ALPHA, dtype=torch.float64)
    else:
        if mode == "var":
            est = d.get_model(Denoiser.SIGMA_ESTIMATOR, False)(xr).mean(dim=(1, 2, 3)).cpu().double()
        else:
            est = d.l_params[Denoiser.ESTIMATED_SIGMA].detach().cpu().double().reshape(1).expand(B)
        alpha_b = (F.softplus(est - 4.0) + 1e-3).clamp(max=0.999)
    loss, pme, mu = impulse_forward_paper(out.cpu().double(), y64, alpha_b, 0.1 if mode != "known" else 0.0)
    L = (loss * w.cpu().double()).sum() + (pme * gp.cpu().double()).sum() + (mu * gm.cpu().double()).sum()
    L.backward()
    torch.cuda.synchronize()
    return xr.grad.cpu().double() + y64.grad


@pytest.mark.parametrize("mode", ["known", "const", "var"])
def test_impulse_x_grad_vs_network_autograd(mode):
    from ssdn.params import PipelineOutput as PO
    B, Psz = 4, 32
    d = impulse_denoiser(mode)
    data = impulse_batch(3, B, Psz)
    g = torch.Generator().manual_seed(23)
    w = torch.randn(B, generator=g).to(DEV)
    gp, gm = (torch.randn(B, 3, Psz, Psz, generator=g) * 1e-2).to(DEV), (torch.randn(B, 3, Psz, Psz, generator=g) * 1e-2).to(DEV)
    want = reference_x_grad(d, mode, data, w, gp, gm)
    x = data[0].detach().clone().requires_grad_(True)
    res = d.run_pipeline([x] + data[1:])
    ((res[PO.LOSS].view(B) * w).sum() + (res[PO.IMG_DENOISED] * gp).sum() + (res[PO.IMG_MU] * gm).sum()).backward()
    torch.cuda.synchronize()
    got = x.grad.cpu().double()
    cos, rel = _cos_rel(got.reshape(-1), want.reshape(-1))
    print("impulse x.grad %s: 1 - cosine %.3e, rel err %.3e" % (mode, 1 - cos, rel))
    assert torch.isfinite(got).all()
    assert 1 - cos <= 2.7e-5 and rel <= 9e-3, (cos, rel)            # tests/test_hip_denoiser_input_grad.py's bounds
    a = res[PO.NOISE_STD_DEV]
    assert tuple(a.shape) == ((1, 1, 1) if mode == "const" else (B, 1, 1))               # alpha, shaped like the gauss styles' sigma
    if mode == "known":
        assert float((a - ALPHA).abs().max()) == 0.0


@pytest.mark.parametrize("mode", ["known", "const", "var"])
def test_impulse_mean_loss_backward_is_bit_identical_and_reproducible(mode):
    from ssdn.params import PipelineOutput as PO
    d = impulse_denoiser(mode)
    data = impulse_batch(3, 4, 32)
    out = d.run_pipeline(data)
    d.backward()
    torch.cuda.synchronize()
    g_ref, loss_ref, pme_ref = d.flat_grad.clone(), out[PO.LOSS].detach().clone(), out[PO.IMG_DENOISED].detach().clone()
    assert torch.isfinite(g_ref).all() and float(g_ref.abs().max()) > 0
    for _ in range(2):                                                # autograd route, twice: bit-identical every time
        d.flat_grad.zero_()
        out = d.run_pipeline(data)
        torch.mean(out[PO.LOSS]).backward()
        torch.cuda.synchronize()
        assert torch.equal(out[PO.LOSS].detach(), loss_ref) and torch.equal(out[PO.IMG_DENOISED].detach(), pme_ref)
        assert torch.equal(d.flat_grad, g_ref), "%d of %d gradient elements differ" % (int((d.flat_grad != g_ref).sum()), g_ref.numel())


class ImpulseCpuTrainer(R.CpuTrainer):
    """the oracle trainer with the fp32 mirror head"""

    def forward(self, noisy, ref=None, noise_param=None, coords=None):
        out = R.net_forward(self.p, noisy, self.blindspot)
        est_raw = None
        if self.mode == "const":
            est_raw = self.est
        elif self.mode == "var":
            est_raw = R.net_forward(self.ps, noisy, False).mean(dim=(2, 3), keepdim=True)
        B = noisy.shape[0]
        m = impulse_head(out, noisy, noise_param.reshape(B) if noise_param is not None else None, self.mode, est_raw, dtype=torch.float32)
        return dict(loss=m["loss"].view(B, 1), out=m["pme"], out_mu=m["mu"], net_out=out)


class _GaussCpuTrainer(R.CpuTrainer):
    pass


def _trajectory(style, mode):
    """three Adam steps next to the CPU loop, each from the CPU loop's current state -> per iteration (loss, oracle loss, pme rel err,
    gradient cosine, sign agreement, update cosine, max |update| / lr)"""
    from ssdn.denoiser import Denoiser
    from ssdn.datasets import NoisyDataset
    from ssdn.params import PipelineOutput
    from test_hip_denoiser_autograd import seeded_denoiser
    impulse = style.startswith("impulse")
    d = impulse_denoiser(mode, style=style) if impulse else seeded_denoiser("ssdn", style, mode, 3)
    p0 = R.make_params(3, 9, True, seed=5)
    sp0 = R.make_params(3, 1, False, seed=6) if mode == "var" else None
    tr = (ImpulseCpuTrainer if impulse else _GaussCpuTrainer)("ssdn", 3, style, mode, params=p0, sigma_params=sp0)
    if tr.est is not None:
        with torch.no_grad():
            tr.est.fill_(1.7)
    nets = [(d.get_model(Denoiser.MODEL, False), 0, tr.p)]
    if sp0 is not None:
        nets.append((d.get_model(Denoiser.SIGMA_ESTIMATOR, False), d._n_main, tr.ps))
    noisy, clean, _ = impulse_batch(3, 2, 32, seed=3, dev=False)          # the same seeds (and the same images) for either style
    npar = torch.full((2, 1, 1, 1), ALPHA if impulse else 25 / 255.0)
    meta = {NoisyDataset.Metadata.INPUT_NOISE_VALUES: npar, NoisyDataset.Metadata.CLEAN: clean}
    rows = []
    for it in range(3):
        lr = R.trainer_lr((it + 1) * 40, 1000)
        start = _flat_of(d, nets, tr)
        d.flat.copy_(start)
        d.adam_m.copy_(_cat_state(d, nets, tr, tr.m))
        d.adam_v.copy_(_cat_state(d, nets, tr, tr.v))
        d.adam_steps = tr.steps
        d.mark_dirty()
        out = d.run_pipeline([noisy, clean, meta])
        d.backward()
        for t in tr.leaves:
            t.grad = None
        r = tr.forward(noisy, clean, npar, None)
        r["loss"].mean().backward()
        loss = out[PipelineOutput.LOSS].detach().cpu().numpy().reshape(-1)
        o = out[PipelineOutput.IMG_DENOISED].detach().cpu()
        prel = float((o - r["out"].detach()).norm() / r["out"].detach().norm())
        gd, gr = d.flat_grad.cpu(), _flat_grad_of(d, nets, tr)
        cos = float((gd * gr).sum() / (gd.norm() * gr.norm() + 1e-30))
        agree = float(((gd > 0) == (gr > 0)).float().mean())
        d.optimizer_step(lr)
        tr.steps += 1
        with torch.no_grad():
            for t, m, v in zip(tr.leaves, tr.m, tr.v):
                R.adam_step(t, t.grad, m, v, tr.steps, lr)
        torch.cuda.synchronize()
        du, ru = d.flat.cpu() - start, _flat_of(d, nets, tr) - start
        ucos = float((du * ru).sum() / (du.norm() * ru.norm() + 1e-30))
        rows.append(dict(loss=loss, oracle=r["loss"].detach().numpy().reshape(-1), prel=prel, cos=cos, agree=agree, ucos=ucos,
                         umax=float(du.abs().max()) / lr))
        print("%s/%s iteration %d: loss %s (CPU loop %s), pme rel err %.3e, gradient 1 - cosine %.3e, sign agreement %.4f, update cosine %.4f"
              % (style, mode, it, loss.tolist(), rows[-1]["oracle"].tolist(), prel, 1 - cos, agree, ucos))
    return rows


@pytest.mark.parametrize("mode", ["known", "const", "var"])
def test_impulse_training_trajectory(mode):
    """tests/test_hip_diag_cov.py::test_diag_training_trajectory's bounds for impulse50.  Where the gradient cosine misses 0.997 the
    gauss25 model is measured at the same seeds in the same run: the impulse shortfall 1 - cos may be at most twice gauss25's."""
    rows = _trajectory("impulse50", mode)
    gauss = None
    for it, r in enumerate(rows):
        np.testing.assert_allclose(r["loss"], r["oracle"], rtol=1e-2, atol=2e-3, err_msg="loss, iteration %d" % it)
        if it == 0:
            assert r["prel"] <= 1e-2, r["prel"]
        bound = 1 - 0.997
        if 1 - r["cos"] > bound:
            gauss = gauss or _trajectory("gauss25", mode)
            print("iteration %d: impulse 1 - cos %.3e, gauss25 1 - cos %.3e" % (it, 1 - r["cos"], 1 - gauss[it]["cos"]))
            bound = max(bound, 2 * (1 - gauss[it]["cos"]))
        assert 1 - r["cos"] <= bound and r["agree"] >= 0.97, "iteration %d: gradient cosine %.4f, sign agreement %.4f" % (it, r["cos"], r["agree"])
        assert r["ucos"] >= 0.95, "iteration %d: Adam update cosine %.4f" % (it, r["ucos"])
        assert r["umax"] <= 3.5


def test_impulse_eval_forward_and_wt_round_trip(tmp_path):
    """Evaluation at 256x256, the head teacher-forced on the network output the engine computed; after training steps a `.wt` reloads
    through DenoiserEvaluator with the same outputs"""
    from ssdn.datasets import NoisyDataset
    from ssdn.eval import DenoiserEvaluator
    from ssdn.params import PipelineOutput as PO
    d = impulse_denoiser("known")
    S = 256
    x, clean, _ = impulse_batch(3, 1, S, seed=7)
    npar = torch.full((1, 1, 1, 1), ALPHA)
    meta = {NoisyDataset.Metadata.INPUT_NOISE_VALUES: npar}
    d.eval()
    with torch.no_grad():
        out = d.run_pipeline([x, None, meta])
    tr = ImpulseCpuTrainer("ssdn", 3, "impulse50", "known", params=R.make_params(3, 9, True, seed=5))
    with torch.no_grad():
        r = tr.forward(x.cpu(), None, npar)
    rel_mu = float((out[PO.IMG_MU].cpu() - r["out_mu"]).norm() / r["out_mu"].norm())
    rel = float((out[PO.IMG_DENOISED].cpu() - r["out"]).norm() / r["out"].norm())
    print("impulse eval 256x256: PME rel err %.3e, mu rel err %.3e" % (rel, rel_mu))
    assert rel_mu <= 5e-3 and rel <= 1e-2, (rel_mu, rel)
    eng = d._last_engine
    t = impulse_head(eng.main.tensor("out32").cpu(), x.cpu(), npar.view(1), "known", None)
    fig = _fp32_yardstick(eng.main.tensor("out32").cpu(), x.cpu(), npar.view(1), "known", None, t)
    close(eng.pme, t["pme"], 2e-5, _atol(5e-6, fig["pme"]), "eval PME, teacher-forced")
    close(eng.model_std, t["model_std"], 2e-5, 1e-6, "eval model std, teacher-forced")
    close(eng.loss.view(-1), t["loss"], 2e-5, 1e-6, "eval loss, teacher-forced")
    d.train()
    data = impulse_batch(3, 4, 32)
    for _ in range(3):
        d.train_step(data, lr=3e-4)
    d.eval()
    with torch.no_grad():
        want = d.run_pipeline([x, None, meta])
    sd = {k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in d.state_dict().items()}
    torch.save(sd, tmp_path / "model.wt")
    ev = DenoiserEvaluator(str(tmp_path / "model.wt"), runs_dir=str(tmp_path / "runs"))
    assert "impulse50" in ev.denoiser.config_name()
    ev.denoiser.eval()
    with torch.no_grad():
        got = ev.denoiser.run_pipeline([x, None, meta])
    for k in (PO.IMG_DENOISED, PO.IMG_MU, PO.MODEL_STD_DEV, PO.NOISE_STD_DEV):
        assert torch.equal(got[k], want[k]), k


def test_impulse_plan_blob_through_the_c_abi_alone_is_bit_identical(tmp_path):
    """config 2's shape (batch 32, 64x64, sigma_known) with the impulse head: the exported blob, run by the unchanged
    tests/plan_c_driver.py in a separate process, gives the Python engine's losses, parameters and posterior mean bit for bit"""
    from ssdn.hip import lib as L
    from ssdn.params import PipelineOutput
    noisy, clean, meta = impulse_batch(3, 32, 64, seed=9, dev=False)
    npar = torch.full((32, 1, 1, 1), ALPHA)
    torch.manual_seed(21)
    d = impulse_denoiser("known", seeded=False)
    params0 = d.flat.detach().cpu().clone()
    lr, steps = 3e-4, 2
    losses = []
    for _ in range(steps):
        out = d.train_step([noisy, clean, meta], lr)
        torch.cuda.synchronize()
        losses.append(out[PipelineOutput.LOSS].detach().cpu().reshape(-1).clone())
    eng = d._last_train_engine
    blob = eng.export_plan(dict(config="config 2's shape, impulse50"))
    (tmp_path / "plan.bin").write_bytes(blob)
    torch.save(dict(params=params0, noisy=noisy, noise_param=npar.reshape(-1), ref=None, coords=None, lr=lr, steps=steps), tmp_path / "in.pt")
    env = dict(os.environ)
    env.pop("PYTHONPATH", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "plan_c_driver.py"), L.LIB_PATH, str(tmp_path / "plan.bin"),
                        str(tmp_path / "in.pt"), str(tmp_path / "out.pt")], capture_output=True, text=True, timeout=600, cwd=str(tmp_path), env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    got = torch.load(tmp_path / "out.pt")
    assert got["meta"]["style"] == "impulse" and got["meta"]["pipeline"] == "ssdn"
    for a, b in zip(losses, got["loss"]):
        assert torch.isfinite(a).all() and torch.equal(a, b.reshape(-1)), (a[:4], b.reshape(-1)[:4])
    n = d.flat.numel()
    assert torch.equal(d.flat.detach().cpu(), got["params"][:n]), "parameters after two steps through the C ABI differ"
    assert torch.equal(eng.pme.cpu().reshape(-1), got["pme"])


def test_impulse_accumulated_halves_are_the_ordered_fp32_sum():
    """mode const (the staged scalar): two accumulated micro-batches leave fl(g_0 + g_1), torch.equal"""
    d = impulse_denoiser("const")
    data = [impulse_batch(3, 4, 64, seed=10 * k) for k in range(2)]
    gs = []
    for k in range(2):
        d.run_pipeline(data[k])
        d.backward()
        gs.append(d.flat_grad.clone())
    assert all(torch.isfinite(g).all() for g in gs) and not torch.equal(gs[0], gs[1]) and float(gs[0].abs().max()) > 0
    o = d._n_main + d._n_sig
    assert float(gs[0][o]) != 0.0 and float(gs[1][o]) != 0.0               # the learnt alpha has a gradient
    want = gs[0] + gs[1]
    d.zero_grad()
    for k in range(2):
        d.accumulate_step(data[k])
    torch.cuda.synchronize()
    assert torch.equal(d.flat_grad, want)
    d.accumulate_grads = True
    d.zero_grad()
    for k in range(2):
        d.run_pipeline(data[k])
        d.backward()
    assert torch.equal(d.flat_grad, want)


# ---- 5. the trainer ---------------------------------------------------------------------------------------------------------------------------------
def test_cli_train_impulse_resume_eval_round_trip(tmp_path):
    """`ssdn train start -n impulse50` over the HDF5 fixture, resume, eval: the device stream corrupts the training patches (style 2), the
    host `add_impulse` the evaluation set"""
    from ssdn.__main__ import start_cli
    from ssdn.params import ConfigValue, StateValue
    h5 = os.path.join(ROOT, "tests", "golden", "g_libhdf5_dataset.h5")
    runs = str(tmp_path / "runs")
    torch.manual_seed(20261017)
    tr = start_cli(["train", "start", "-a", "ssdn", "-n", "impulse50", "--noise_value", "const", "-t", h5, "-v", h5, "-i", "64",
                    "--train_batch_size", "8", "--validation_batch_size", "2", "--patch_size", "32", "--eval_interval", "32",
                    "--print_interval", "16", "--checkpoint_interval", "32", "--runs_dir", runs])
    run = tr.run_dir_path
    assert "ssdn-impulse50-sigma_const" in os.path.basename(run) and tr.state[StateValue.ITERATION] == 64
    assert "TRAINING FINISHED" in open(os.path.join(run, "log.txt")).read()
    rows = list(csv.DictReader(open(os.path.join(run, "scalars.csv"))))
    sc = {}
    for r in rows:
        sc.setdefault(r["tag"], []).append((int(r["step"]), float(r["value"])))
    assert [s for s, _ in sc["train/loss"]] == [16, 32, 48, 64] and all(np.isfinite(v) for _, v in sc["train/loss"])
    nstd = [k for k in sc if k.startswith("train/") and "noise" in k]
    assert nstd and all(0.255 <= v <= 254.8 for _, v in sc[nstd[0]])        # the "noise std" metric reads 255 * alpha
    assert "valid/psnr_out" in sc and all(np.isfinite(v) for _, v in sc["valid/psnr_out"])
    t2 = start_cli(["train", "resume", run, "-i", "96"])
    assert t2.run_dir_path == run and t2.state[StateValue.ITERATION] == 96
    assert t2.cfg[ConfigValue.NOISE_STYLE] == "impulse50"
    wt = glob.glob(os.path.join(run, "final-*.wt"))
    assert len(wt) == 1 and "impulse50" in os.path.basename(wt[0])
    ev = start_cli(["eval", "-m", wt[0], "-d", h5, "--runs_dir", runs, "--batch_size", "1"])
    prow = list(csv.DictReader(open(os.path.join(ev.run_dir_path, "psnrs.csv"))))
    assert len(prow) == 5 and all(np.isfinite(float(r["psnr_out"])) for r in prow)
    assert all(float(r["psnr_nsy"]) < 20.0 for r in prow)                   # half of the pixels replaced: the input is bad
