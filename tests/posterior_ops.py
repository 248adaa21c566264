"""SSDN_OP_HEAD_POSTERIOR as the GPU tests launch it: through ctypes on device copies of host tensors (head_ops.py's manner), for every
style (gauss*, poisson*, impulse*), the full and the diagonal head.  Every output buffer is NaN-poisoned before the launch and returned
whether it was requested or not, so an element the kernel leaves out, or writes without being asked to, shows."""
import torch

from head_ops import DEV, P, _dev, _nan, _style, run_one


def posterior_op(net_out, noisy, npar, style, mode, est_raw, diag=0, nchunks=2, n_samples=0, seed=0, offset=0, want=("cov", "std", "samples")):
    """one launch -> dict of cov [B,C(C+1)/2,H,W], std [B,C,H,W], samples [max(n_samples, 1),B,C,H,W] (device tensors); `want`: the outputs
    whose pointers are passed (samples only with n_samples > 0)"""
    from ssdn.hip import lib as L
    from ssdn.hip.engine import MODE
    B, _, H, W = net_out.shape
    C = noisy.shape[1]
    no, y, npd, er = _dev(net_out), _dev(noisy), _dev(npar), _dev(est_raw)
    cov, std, smp = _nan(B, C * (C + 1) // 2, H, W), _nan(B, C, H, W), _nan(max(n_samples, 1), B, C, H, W)
    a = L.HeadPosteriorArgs(P(no), P(y), P(npd), P(er), B, C, H, W, _style(style), MODE[mode], diag, nchunks,
                            P(cov) if "cov" in want else None, P(std) if "std" in want else None,
                            P(smp) if "samples" in want and n_samples > 0 else None, n_samples, seed, offset)
    run_one("head_posterior", a)
    return dict(cov=cov, std=std, samples=smp)
