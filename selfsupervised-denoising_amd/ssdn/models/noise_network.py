"""`NoiseNetwork` -- the (optionally blind-spot) U-Net of the ssdn package, MI355X edition.

Same constructor, `forward`, `blindspot`, `init_weights`, `input_wh_mul` and `state_dict` layout as the reference module
(/root/reference/ssdn/ssdn/models/noise_network.py:13-238), but it is NOT a stack of torch.nn layers: the module only
owns the parameters (as views into one flat fp32 buffer, the layout the fused Adam / RCCL all-reduce work on) and
`forward` executes the planned op list of `ssdn.hip.graph.NetPlan` through libssdn_hip.so.  There is no eager / CPU
fallback: without the HIP library or a GPU `forward` raises.

Autograd: when a gradient is wanted (grad mode on, and `x` or any parameter requires grad) `forward` runs a TRAINING plan through
a torch.autograd.Function; its backward copies dL/d(out) into the plan's upstream-gradient buffer and runs the planned backward list
-- every weight gradient, plus d/dx (SSDN_OP_INPUT_GRAD) when `x` requires grad.  Parameter gradients come from one fresh copy of a
module-owned flat gradient buffer, so `.grad` accumulates through torch's AccumulateGrad as for any module.  The plan's activations
are shared by every grad-mode call of the same input shape: a backward after a second grad-mode forward of that shape raises
RuntimeError, as does a backward after an in-place parameter update (torch's version check) or a double backward.  Otherwise
(torch.no_grad(), or nothing requires grad) `forward` runs the forward-only plan and returns a tensor without a graph.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn
from torch import Tensor
from torch.autograd.function import once_differentiable

from ssdn.hip.graph import net_layers, net_param_count


class _ConvParams(nn.Module):
    """Parameter holder standing where the reference has an nn.Conv2d / ShiftConv2d (same key names, OIHW weight)."""

    def __init__(self, weight: Tensor, bias: Tensor):
        super().__init__()
        self.weight = nn.Parameter(weight, requires_grad=True)
        self.bias = nn.Parameter(bias, requires_grad=True)


class _Slots(nn.Module):
    """nn.Sequential-like container whose children keep the reference's numeric names ('0', '2', '4')."""

    def __init__(self, children: Dict[str, nn.Module]):
        super().__init__()
        for k, m in children.items():
            self.add_module(k, m)


class _NetFunction(torch.autograd.Function):
    """out = net(x) on a training plan; backward = the plan's backward list (+ SSDN_OP_INPUT_GRAD when x needs a gradient)."""

    @staticmethod
    def forward(ctx, net: "NoiseNetwork", x: Tensor, *params: Tensor) -> Tensor:
        slot, out = net._run_grad_forward(x, input_grad=ctx.needs_input_grad[1])
        ctx.slot, ctx.gen = slot, slot[2]
        ctx.x_device, ctx.x_dtype = x.device, x.dtype
        ctx.offsets = [net._param_offset(p) for p in params]
        ctx.save_for_backward(*params)         # (torch's version check: an in-place update of a parameter before backward raises)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out: Tensor):
        from ssdn.hip.engine import current_stream
        params = ctx.saved_tensors
        eng = ctx.slot[0]
        if ctx.slot[2] != ctx.gen:
            raise RuntimeError("NoiseNetwork: the activations of this graph were overwritten by a later grad-mode forward of the same "
                               "input shape; run backward before the next forward of that shape")
        eng.tensor("g32").copy_(grad_out.to(dtype=torch.float32))
        eng.bwd.run(current_stream())
        dx = None
        if ctx.needs_input_grad[1]:
            dx = eng.tensor("dx32").clone().to(device=ctx.x_device, dtype=ctx.x_dtype)
        grads = [None] * len(params)
        if any(ctx.needs_input_grad[2:]):
            flat = eng.grads.clone()           # one copy: the next backward overwrites the engine's buffer
            for i, (p, off) in enumerate(zip(params, ctx.offsets)):
                if ctx.needs_input_grad[2 + i]:
                    grads[i] = flat[off:off + p.numel()].view(p.shape)
        return (None, dx, *grads)


class NoiseNetwork(nn.Module):
    def __init__(self, in_channels: int = 3, out_channels: int = 3, blindspot: bool = False,
                 zero_output_weights: bool = False, device: Optional[torch.device] = None,
                 flat: Optional[Tuple[Tensor, Optional[Tensor]]] = None):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self._blindspot = blindspot
        self._zero_output_weights = zero_output_weights
        self.layers = net_layers(in_channels, out_channels, blindspot)
        self.nparams = net_param_count(self.layers)
        if device is None:
            device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self._device = torch.device(device)
        if flat is None:
            flat = (torch.zeros(self.nparams, device=self._device), None)
        self._flat, self._flat_grad = flat
        assert self._flat.numel() == self.nparams
        # parameter views + the reference's module tree (noise_network.py:69-156)
        holders = OrderedDict()
        for l in self.layers:
            w = self._flat[l.w_off:l.w_off + l.M * l.cin * l.k * l.k].view(l.M, l.cin, l.k, l.k)
            b = self._flat[l.b_off:l.b_off + l.M]
            holders[l.name] = _ConvParams(w, b)
        blocks = OrderedDict()
        for name, h in holders.items():
            blk, idx = name.split(".")
            blocks.setdefault(blk, OrderedDict())[idx] = h
        for blk in ("encode_block_1", "encode_block_2", "encode_block_3", "encode_block_4", "encode_block_5", "encode_block_6",
                    "decode_block_5", "decode_block_4", "decode_block_3", "decode_block_2", "decode_block_1"):
            self.add_module(blk, _Slots(blocks[blk]))
        self.output_conv = blocks["output_block"]["4"]          # alias: ONE parameter under two names (noise_network.py:149-156)
        self.output_block = _Slots(blocks["output_block"])
        # (B, H, W) -> [DeviceNet, parameter version its shadows hold] (forward-only plans);
        # (B, H, W, input_grad) -> [DeviceNet, parameter version, generation] (training plans of the autograd path)
        self._engines: Dict[tuple, list] = {}
        self._grad_buf: Optional[Tensor] = None                # flat gradient the training plans' reductions write
        self._version = 0
        self._consume_default_init_draws()
        self.init_weights()

    # ---- reference surface ----------------------------------------------------------------------------------
    @property
    def blindspot(self) -> bool:
        return self._blindspot

    @staticmethod
    def input_wh_mul() -> int:
        """Inputs must be multiples of 2^5 in both dimensions (five pooling levels, noise_network.py:228-238)."""
        return 32

    def _consume_default_init_draws(self):
        """The reference builds nn.Conv2d modules, whose constructors draw a default (uniform) initialisation for every
        weight and bias from the global generator BEFORE init_weights() overwrites them (noise_network.py:69-159).  Those
        numbers are never used, but they advance the generator; drawing the same amounts in the same construction order keeps
        `torch.manual_seed(s); NoiseNetwork(...)` bit-identical to the reference (tests/test_dropin_surface.py)."""
        by_name = {l.name: l for l in self.layers}
        order = [l for l in self.layers if not l.name.startswith("output_block")]
        order += [by_name["output_block.4"], by_name["output_block.0"], by_name["output_block.2"]]   # output_conv is built first
        for l in order:
            torch.empty(l.M, l.cin, l.k, l.k).uniform_(-1, 1)
            torch.empty(l.M).uniform_(-1, 1)

    def init_weights(self):
        """He-normal for LeakyReLU(0.1) on every conv, zero biases; last layer 'linear' gain or zeros
        (noise_network.py:165-184).  Draws from the global CPU generator in the reference's module order, with the
        reference's shapes, so the same torch seed gives the same network."""
        order = [l for l in self.layers if not l.name.startswith("output_block")]
        ob = {l.name: l for l in self.layers if l.name.startswith("output_block")}
        order += [ob["output_block.4"], ob["output_block.0"], ob["output_block.2"]]   # output_conv is visited first
        with torch.no_grad():
            new = torch.zeros(self.nparams)
            for l in order:
                fan_in = l.cin * l.k * l.k
                std = math.sqrt(2.0 / (1 + 0.1 ** 2)) / math.sqrt(fan_in)
                new[l.w_off:l.w_off + l.M * fan_in] = torch.empty(l.M, l.cin, l.k, l.k).normal_(0, std).reshape(-1)
            last = ob["output_block.4"]
            n_last = last.M * last.cin
            if self._zero_output_weights:
                new[last.w_off:last.w_off + n_last] = 0
            else:
                new[last.w_off:last.w_off + n_last] = torch.empty(last.M, last.cin, 1, 1).normal_(0, 1.0 / math.sqrt(last.cin)).reshape(-1)
            self._flat.copy_(new)
        self.mark_dirty()

    def mark_dirty(self):
        """Parameters changed outside the fused optimiser: the fp16 MFMA shadows must be re-packed before the next run."""
        self._version += 1

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self.mark_dirty()

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        r = super().load_state_dict(state_dict, strict=strict, **kw)
        self.mark_dirty()
        return r

    # ---- execution --------------------------------------------------------------------------------------------
    def _engine(self, B: int, H: int, W: int, train: bool = False, input_grad: bool = False):
        from ssdn.hip import lib as L
        from ssdn.hip.engine import DeviceNet
        from ssdn.hip.graph import NetPlan
        if self._flat.device.type != "cuda":
            raise L.SsdnHipError("NoiseNetwork.forward needs an MI355X: parameters live on %s and the ssdn hot path has no CPU "
                                 "fallback" % self._flat.device)
        key = (B, H, W, bool(input_grad)) if train else (B, H, W)
        if key not in self._engines:
            cus = L.load().ssdn_device_cus()
            plan = NetPlan("n/", self.in_channels, self.out_channels, self._blindspot, B, H, W, cus=cus, train=train,
                           input_grad=bool(input_grad))
            if train and self._grad_buf is None:
                self._grad_buf = torch.zeros(self.nparams, device=self._flat.device)
            self._engines[key] = [DeviceNet(plan, self._flat.device, self._flat, self._grad_buf if train else None), None, 0]
            while len(self._engines) > 4:                  # LRU cap: a plan owns all its activation buffers
                self._engines.pop(next(k for k in self._engines if k != key))
        slot = self._engines.pop(key)
        self._engines[key] = slot
        return slot

    def _param_offset(self, p: Tensor) -> int:
        """offset (floats) of a parameter inside the flat buffer"""
        off = (p.data_ptr() - self._flat.data_ptr()) // 4
        if p.untyped_storage().data_ptr() != self._flat.untyped_storage().data_ptr() or not 0 <= off <= self.nparams - p.numel():
            raise RuntimeError("NoiseNetwork: a parameter no longer lives in the module's flat buffer")
        return off

    def _run_grad_forward(self, x: Tensor, input_grad: bool):
        """forward on the training plan of x's shape (its activations stay for the backward list); -> (engine slot, output)"""
        from ssdn.hip.engine import current_stream
        B, _, H, W = x.shape
        slot = self._engine(B, H, W, train=True, input_grad=input_grad)
        eng = slot[0]
        s = current_stream()
        eng.pack.run(s)                        # (fp16 forward and bf16 data-gradient shadows, as in the forward-only path)
        slot[1] = (self._version, self._flat._version)
        slot[2] += 1                           # generation: a graph made by an earlier forward of this engine can no longer backward
        eng.tensor("in32").copy_(x.to(dtype=torch.float32), non_blocking=True)
        eng.fwd.run(s)
        return slot, eng.tensor("out32").clone()

    def forward(self, x: Tensor) -> Tensor:
        """x: float32 [B,C,H,W] (H, W multiples of 32; square when blindspot) -> float32 [B,out_channels,H,W] on the GPU.
        Differentiable w.r.t. x and the parameters when grad mode is on (module docstring)."""
        from ssdn.hip.engine import current_stream
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise ValueError("expected input [B,%d,H,W], got %s" % (self.in_channels, tuple(x.shape)))
        if torch.is_grad_enabled():
            params = list(self.parameters())
            if x.requires_grad or any(p.requires_grad for p in params):
                return _NetFunction.apply(self, x, *params)
        B, _, H, W = x.shape
        slot = self._engine(B, H, W)
        eng = slot[0]
        s = current_stream()
        # the fp16 shadows are re-packed on every call of this (forward-only) entry point: 23 us, and a write through `p.data`
        # -- which moves neither counter -- can then never leave a stale shadow behind
        eng.pack.run(s)
        slot[1] = (self._version, self._flat._version)
        eng.tensor("in32").copy_(x.to(dtype=torch.float32), non_blocking=True)
        eng.fwd.run(s)
        return eng.tensor("out32").clone()
