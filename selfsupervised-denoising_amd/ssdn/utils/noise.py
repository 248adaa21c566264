"""Noise models of the data layer (drop-in for /root/reference/ssdn/ssdn/utils/noise.py:14-153): `add_style(images, style)`
with the style grammar 'gauss{SD}', 'gauss{MIN}_{MAX}', 'poisson{LAMBDA}', 'poisson{MIN}_{MAX}', 'impulse{A}', 'impulse{LO}_{HI}',
optional '_nc' (no clip); integer parameters of gauss styles are /255, integer parameters of impulse styles are per cent ('impulse50':
alpha = 0.5; with a decimal point they are fractions).  Works on CPU tensors (the reference's per-item dataset path) AND on device
tensors (the batched patch stream, ssdn.datasets.patch_stream: noise is drawn where the batch already lives).

Reference quirks kept: Poisson noise is RATE-1 noise added to lambda*x (utils/noise.py:101-104), not
Poisson(lambda*x); a range style draws one parameter per leading-axis entry of whatever it is called on -- per CHANNEL when
called on an unbatched CHW image (noise.py:55-56), per SAMPLE when called on a batch.

Impulse noise (Laine et al.'s third model; the reference package has no such branch): with probability alpha a PIXEL is replaced, in
all channels jointly, by a colour uniform on [0,1)^C, otherwise it is left exactly as it is.  The decision is one draw per pixel, so a
ranged alpha is one draw per IMAGE (never per channel), and '_nc' changes nothing: every value is in range already."""
import re
from numbers import Number
from typing import Tuple, Union

import torch
from torch import Tensor

from ssdn.utils.data import clip_img


def _range_param(tensor: Tensor, lo, hi, generator=None):
    shape = [tensor.shape[0]] + [1] * (tensor.dim() - 1)
    return lo + (hi - lo) * torch.rand(shape, device=tensor.device, generator=generator)


def add_gaussian(tensor: Tensor, std_dev, mean: Number = 0, inplace: bool = False, clip: bool = True, generator=None):
    if not inplace:
        tensor = tensor.clone()
    if isinstance(std_dev, (list, tuple)):
        if len(std_dev) == 1:
            std_dev = std_dev[0]
        else:
            lo, hi = std_dev
            lo = lo / 255 if isinstance(lo, int) else lo
            hi = hi / 255 if isinstance(hi, int) else hi
            std_dev = _range_param(tensor, lo, hi, generator)
    if isinstance(std_dev, int):
        std_dev = std_dev / 255
    tensor.add_(torch.randn(tensor.shape, device=tensor.device, generator=generator) * std_dev + mean)
    if clip:
        tensor = clip_img(tensor, inplace=True)
    return tensor, std_dev


def add_poisson(tensor: Tensor, lam, inplace: bool = False, clip: bool = True, generator=None):
    if not inplace:
        tensor = tensor.clone()
    if isinstance(lam, (list, tuple)):
        lam = lam[0] if len(lam) == 1 else _range_param(tensor, lam[0], lam[1], generator)
    tensor.mul_(lam)
    noise = torch.poisson(torch.ones(tensor.shape, device=tensor.device, dtype=torch.float64), generator=generator)
    tensor.add_(noise.to(tensor.dtype))
    tensor.div_(lam)
    if clip:
        tensor = clip_img(tensor, inplace=True)
    return tensor, lam


def impulse_alpha(value):
    """a parameter of an impulse style as a fraction: integers are per cent"""
    return value / 100 if isinstance(value, int) else float(value)


def add_impulse(tensor: Tensor, alpha, inplace: bool = False, clip: bool = True, generator=None):
    """tensor: CHW or BCHW.  alpha: a fraction, or [A] / [LO, HI] as `parse_style` returns them (integers per cent).  Returns the
    corrupted tensor and alpha: a number, or for a range the value drawn for each image (CHW: shape [1,1,1]; BCHW: [B,1,1,1])."""
    if tensor.dim() not in (3, 4):
        raise ValueError("add_impulse: CHW or BCHW expected")
    if not inplace:
        tensor = tensor.clone()
    ch = tensor.dim() - 3                               # the channel axis
    lead = [tensor.shape[0]] if ch else []
    if isinstance(alpha, (list, tuple)):
        if len(alpha) == 1:
            alpha = impulse_alpha(alpha[0])
        else:
            lo, hi = impulse_alpha(alpha[0]), impulse_alpha(alpha[1])
            alpha = lo + (hi - lo) * torch.rand(lead + [1, 1, 1], device=tensor.device, generator=generator)
    elif isinstance(alpha, int):
        alpha = impulse_alpha(alpha)
    lo_, hi_ = (float(alpha.min()), float(alpha.max())) if torch.is_tensor(alpha) else (alpha, alpha)
    if not (0.0 <= lo_ and hi_ <= 1.0):
        raise ValueError("impulse noise: alpha must be inside [0, 1]")
    mask_shape = list(tensor.shape)
    mask_shape[ch] = 1                                  # one decision per pixel, shared by the channels
    mask = torch.rand(mask_shape, device=tensor.device, generator=generator) < alpha
    colour = torch.rand(tensor.shape, device=tensor.device, generator=generator).to(tensor.dtype)
    tensor.copy_(torch.where(mask, colour, tensor))
    return tensor, alpha


def parse_style(style: str):
    """'gauss5_50_nc' -> ('gauss', [5, 50], clip=False)"""
    noise_type = re.findall(r"[a-zA-Z]+", style)[0]
    params = style.replace(noise_type, "").split("_")
    clip = "nc" not in params
    params = [p for p in params if p not in ("nc", "")]
    params = [float(p) for p in params] if any("." in p for p in params) else [int(p) for p in params]
    return noise_type, params, clip


def add_style(images: Tensor, style: str, inplace: bool = False, generator=None) -> Tuple[Tensor, Union[Number, Tensor]]:
    noise_type, params, clip = parse_style(style)
    if noise_type == "gauss":
        return add_gaussian(images, params, inplace=inplace, clip=clip, generator=generator)
    if noise_type == "poisson":
        return add_poisson(images, params, inplace=inplace, clip=clip, generator=generator)
    if noise_type == "impulse":
        return add_impulse(images, params, inplace=inplace, clip=clip, generator=generator)
    raise NotImplementedError("Noise type not supported")
