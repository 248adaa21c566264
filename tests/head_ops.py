"""The loss-head ops as the GPU tests launch them: SSDN_OP_HEAD_SSDN + SSDN_OP_HEAD_FINAL (head_op) and SSDN_OP_HEAD_VJP (head_vjp_op)
through ctypes, on device copies of host tensors, for every style (gauss*, poisson*, impulse*), the full and the diagonal head.
Every output is NaN-poisoned before the launch unless an `*_init` is given, so an element the kernel leaves out shows; g_est starts at
zero (the kernels write one entry of it in mode const) and the partials of a vector-Jacobian product start at zero or at `partial_init`."""
import torch

DEV = torch.device("cuda:0")


def P(t):
    return t.data_ptr() if t is not None else None


def run_one(ty, args):
    from ssdn.hip.engine import OpList, current_stream
    OpList([(ty, args)]).run(current_stream())
    torch.cuda.synchronize()


def _dev(t):
    return None if t is None else t.to(DEV, torch.float32).contiguous()


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _style(style):
    from ssdn.hip.engine import STYLE
    return 2 if style.startswith("impulse") else STYLE["poisson" if style.startswith("poisson") else "gauss"]


def head_op(net_out, noisy, npar, style, mode, est_raw, diag=0, nchunks=2, want_grad=1):
    """one forward launch and its reduction -> dict of loss, mu, pme, model_std, noise_std ([B,H,W] for poisson, [B] otherwise),
    g_net_out, partial, g_est, g_sig, gmax"""
    from ssdn.hip import lib as L
    from ssdn.hip.engine import MODE
    B, Cout, H, W = net_out.shape
    C = noisy.shape[1]
    no, y, npd, er = _dev(net_out), _dev(noisy), _dev(npar), _dev(est_raw)
    mu, pme, mstd, gno = _nan(B, C, H, W), _nan(B, C, H, W), _nan(B, H, W), _nan(B, Cout, H, W)
    nstd = _nan(B, H, W) if style.startswith("poisson") else _nan(B)
    partial = _nan(B, nchunks, 2)
    gmax = torch.zeros(4, dtype=torch.int32, device=DEV)
    run_one("head_ssdn", L.HeadArgs(P(no), P(y), P(npd), P(er), B, C, H, W, _style(style), MODE[mode], want_grad, P(mu), P(pme), P(mstd),
                                    P(nstd), P(gno), P(partial), nchunks, P(gmax), diag))
    loss, g_est = _nan(B), torch.zeros(B, dtype=torch.float32, device=DEV)
    g_sig, gmax2 = _nan(B, 1, H, W), torch.zeros(4, dtype=torch.int32, device=DEV)
    grad = bool(want_grad)
    run_one("head_final", L.HeadFinalArgs(P(partial), B, nchunks, H, W, MODE[mode], P(loss), P(g_est) if grad and mode != "known" else None,
                                          P(g_sig) if grad and mode == "var" else None, P(gmax2) if grad and mode == "var" else None))
    return dict(loss=loss, mu=mu, pme=pme, model_std=mstd, noise_std=nstd, g_net_out=gno, partial=partial, g_est=g_est, g_sig=g_sig,
                gmax=gmax)


def head_vjp_op(net_out, noisy, npar, style, mode, est_raw, w, gp, gm, diag=0, keep=0, nchunks=2, g_noisy=True, g_init=None,
                partial_init=None):
    """one SSDN_OP_HEAD_VJP launch -> dict of g_net_out, partial, g_est and g_sig (None where the mode has none), g_noisy (None when
    not requested), gmax"""
    from ssdn.hip import lib as L
    from ssdn.hip.engine import MODE
    B, Cout, H, W = net_out.shape
    C = noisy.shape[1]
    gno = _nan(B, Cout, H, W) if g_init is None else g_init.to(DEV).clone()
    partial = torch.zeros(B, nchunks, 2, dtype=torch.float32, device=DEV) if partial_init is None else partial_init.to(DEV).clone()
    g_est = torch.zeros(B, dtype=torch.float32, device=DEV) if mode != "known" else None
    g_sig = _nan(B, 1, H, W) if mode == "var" else None
    gmax, gmax2 = torch.zeros(4, dtype=torch.int32, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    gy = _nan(B, C, H, W) if g_noisy else None
    ins = [_dev(t) for t in (net_out, noisy, npar, est_raw, w, gp, gm)]
    a = L.HeadVjpArgs(*[P(t) for t in ins[:4]], B, C, H, W, _style(style), MODE[mode], *[P(t) for t in ins[4:]], keep, nchunks, P(gno),
                      P(partial), P(gmax), P(g_est), P(g_sig), P(gmax2))
    a.g_noisy, a.diag = P(gy), diag
    run_one("head_vjp", a)
    return dict(g_net_out=gno, partial=partial, g_est=g_est, g_sig=g_sig, g_noisy=gy, gmax=gmax)
