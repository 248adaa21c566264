"""Device side of the op-list plans: owns the HBM buffers (allocated through torch, used as a plain device allocator),
materialises `ssdn.hip.graph` Op records into the C structs of include/ssdn_hip.h and executes them with ONE call
into libssdn_hip.so per phase (forward / backward / optimiser).  No torch compute op is on this path.  Order and lanes of
the backward list are the planner's (NetPlan.bwd_sched); here the list is only cut (input gradient, deferred tail) and marked (events).
"""
from __future__ import annotations

import os
import ctypes as C
import math
from typing import Dict, List, Optional

import torch

from . import lib as L
from .dp import N_MAIN_BUCKETS, bucket_layers
from .graph import NetPlan, Op, View


def _ptr(t: torch.Tensor, byte_off: int = 0) -> int:
    return t.data_ptr() + byte_off


class OpList:
    """A materialised op list: a ctypes array of ssdn_op plus the argument structs it points to."""

    def __init__(self, recs):
        """recs: (type, args) or (type, args, lane) -- lane 0, the main lane, where none is given"""
        self.args = [r[1] for r in recs]                      # keep the structs alive
        self.arr = (L.OpRec * max(1, len(recs)))()
        for i, r in enumerate(recs):
            self.arr[i].type = L.OP[r[0]]
            self.arr[i].lane = r[2] if len(r) > 2 else 0
            self.arr[i].args = C.cast(C.pointer(r[1]), C.c_void_p)
        self.n = len(recs)

    def run(self, stream: int = 0):
        if self.n:
            L.check(L.load().ssdn_run_ops(self.arr, self.n, C.c_void_p(stream)))


def current_stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _tile_check(name: str, t: torch.Tensor, dtype, numel: int):
    if t.dtype != dtype or not t.is_contiguous() or t.device.type != "cuda" or t.numel() < numel:
        raise L.SsdnHipError("%s must be a contiguous %s device tensor of at least %d elements" % (name, dtype, numel))


def check_white(white, what: str = "white") -> int:
    """`white` of the 16-bit ops (include/ssdn_hip.h): the uint16 sample value that means 1.0; None is the full range"""
    if white is None:
        return L.WHITE_MAX
    if isinstance(white, bool) or int(white) != white or not 1 <= int(white) <= L.WHITE_MAX:
        raise ValueError("%s must be an integer in [1, %d], got %r" % (what, L.WHITE_MAX, white))
    return int(white)


def tile_in(img: torch.Tensor, w: int, h: int, T: int, O: int, k0: int, dst: torch.Tensor, white: Optional[int] = None) -> torch.Tensor:
    """The tiles k0 .. k0 + B - 1 of one image into dst [B,C,T,T] (SSDN_OP_TILE_IN, csrc/tile_io.hip; the tiling is defined in
    include/ssdn_hip.h): one launch on torch's current stream that divides by 255, transposes to the package's swapped axes and reflects
    where a tile reaches past the image.  img: the image's bytes on the device, uint8 [h w C] upright and interleaved; dst: normally an
    inference engine's `inp`, which `Denoiser._run` then takes without a copy.  Belongs to no engine: the image is not of a plan's shape.
    A uint16 img runs SSDN_OP_TILE_IN16 (the same kernel over uint16 samples): min(sample, white) / white, white the sample value that
    means 1.0 (default 65535); white is refused for bytes."""
    B, Cn = int(dst.shape[0]), int(dst.shape[1])
    wide = img.dtype == torch.uint16
    if white is not None and not wide:
        raise L.SsdnHipError("tile_in: white is for uint16 images")
    _tile_check("tile_in: img", img, torch.uint16 if wide else torch.uint8, w * h * Cn)
    _tile_check("tile_in: dst", dst, torch.float32, B * Cn * T * T)
    if tuple(dst.shape) != (B, Cn, T, T):
        raise L.SsdnHipError("tile_in: dst must be [B, C, %d, %d]" % (T, T))
    image = (_ptr(img), img.numel(), w, h, Cn, T, O, L.tile_count(w, T, O), L.tile_count(h, T, O), k0, B)
    if wide:
        rec = ("tile_in16", L.TileIn16Args(*image, check_white(white), _ptr(dst)))
    else:
        rec = ("tile_in", L.TileInArgs(*image, _ptr(dst)))
    OpList([rec]).run(current_stream())
    return dst


def tile_out(store: torch.Tensor, w: int, h: int, T: int, O: int, mode: int, dst: torch.Tensor, white: Optional[int] = None) -> torch.Tensor:
    """The tiles' values of one image blended back into that image (SSDN_OP_TILE_OUT): one launch on torch's current stream.  store:
    fp32 [Kx Ky, C, T, T] on the device; mode 0: dst uint8, the picture's bytes [h, w, C] (clipped, * 255, truncated); mode 1: dst fp32,
    upright planes [C, h, w].  Only the first w h C elements of dst are written.  Does not synchronise.
    A uint16 dst (mode 0 only) runs SSDN_OP_TILE_OUT16: the same blend, clipped, * white, rounded to nearest even (white: default 65535)."""
    Kx, Ky = L.tile_count(w, T, O), L.tile_count(h, T, O)
    Cn = int(store.shape[1])
    if tuple(store.shape) != (Kx * Ky, Cn, T, T):
        raise L.SsdnHipError("tile_out: store must be [%d, C, %d, %d]" % (Kx * Ky, T, T))
    _tile_check("tile_out: store", store, torch.float32, Kx * Ky * Cn * T * T)
    wide = dst.dtype == torch.uint16
    if wide and mode != 0:
        raise L.SsdnHipError("tile_out: a uint16 dst takes mode 0 (the fp32 map is mode 1 into an fp32 dst)")
    if white is not None and not wide:
        raise L.SsdnHipError("tile_out: white is for a uint16 dst")
    _tile_check("tile_out: dst", dst, torch.uint16 if wide else torch.float32 if mode else torch.uint8, w * h * Cn)
    tiles = (_ptr(store), w, h, Cn, T, O, Kx, Ky)
    if wide:
        rec = ("tile_out16", L.TileOut16Args(*tiles, check_white(white), _ptr(dst), dst.numel()))
    else:
        rec = ("tile_out", L.TileOutArgs(*tiles, mode, _ptr(dst), dst.numel() * dst.element_size()))
    OpList([rec]).run(current_stream())
    return dst


class DeviceNet:
    """One NoiseNetwork instance on the device for a fixed input shape: buffers + materialised fwd/bwd/pack op lists."""

    DT = {"act": torch.float16, "actb": torch.bfloat16, "f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32,
          "u32": torch.int32, "i64": torch.int64, "u8": torch.uint8}

    def __init__(self, plan: NetPlan, device, params: torch.Tensor, grads: Optional[torch.Tensor],
                 shared: Optional[Dict[str, torch.Tensor]] = None, hold_input_grad: bool = False):
        self.plan, self.device = plan, device
        self.params, self.grads = params, grads
        self.t: Dict[str, torch.Tensor] = dict(shared or {})
        for name, spec in plan.tensors.items():
            if name in self.t:
                continue
            # zero-initialised once: padding channels / never-written slab corners must be finite, and the rows of `u` that the one-row
            # shift of the un-rotation leaves empty are never written by the fused SSDN_OP_UNROT_FWD (ssdn_conv_args.urot): they ARE these zeros
            self.t[name] = torch.zeros(spec.shape, dtype=self.DT[spec.kind], device=device)
        self.fwd = OpList([self._mat(op) for op in plan.fwd])
        # the backward list in the planner's execution order (plan.bwd_sched): (type, args, lane), and the layer of every slab reduction
        recs = [self._mat(op) for op in plan.bwd]
        self._bwd_recs = [recs[i] + (lane,) for i, lane in plan.bwd_sched]
        self._bwd_layers = [plan.bwd[i].a["layer"] if plan.bwd[i].type == "wreduce" else None for i, _ in plan.bwd_sched]
        # the SSDN_OP_INPUT_GRAD record of an input-gradient plan (its owner may set the addend); hold_input_grad: the op leaves the
        # backward list and runs as `input_grad_ops` where the owner enqueues it (behind a term computed on another stream)
        k = next((i for i, r in enumerate(self._bwd_recs) if r[0] == "input_grad"), None)
        self.input_grad_args = self._bwd_recs[k][1] if k is not None else None
        self.input_grad_ops = None
        if hold_input_grad and k is not None:
            self.input_grad_ops = OpList([self._bwd_recs[k][:2]])
            del self._bwd_recs[k]
            del self._bwd_layers[k]
        self.bwd = OpList(self._bwd_recs)
        # the last gradient bucket's slab reductions close the list: a training step may run them in front of its optimiser launch
        # instead (DeviceEngine.backward(defer_tail=True)): [weight-gradient lane: wait for the main lane's last launch, two
        # reduction launches] -> join -> Adam becomes join -> reductions -> Adam on ONE stream (one cross-lane hop less in the serial tail)
        ntail = 0
        while ntail < len(self._bwd_recs) and self._bwd_recs[len(self._bwd_recs) - 1 - ntail][0] == "wreduce":
            ntail += 1
        self.tail_recs = [(r[0], r[1]) for r in self._bwd_recs[len(self._bwd_recs) - ntail:]] if 0 < ntail < len(self._bwd_recs) else []
        self.bwd_head = OpList(self._bwd_recs[:len(self._bwd_recs) - len(self.tail_recs)]) if self.tail_recs else None
        self.pack = OpList([self._mat(op) for op in plan.pack])
        self.accumulate = False

    def set_accumulate(self, on: bool) -> None:
        """Whether the next backward pass of this network ADDS its weight and bias gradients to the flat gradient (gradient accumulation
        over micro-batches, ssdn_wreduce_args.accumulate) instead of storing them.  A property of a run, not of the plan: set on the
        materialised SSDN_OP_WREDUCE argument structs, in place.  Every variant of the backward list (`bwd`, `bwd_head` + `tail_recs`, the
        optimiser list that carries the deferred tail, a list with event marks) points at these same structs, so none is rebuilt."""
        self.accumulate = bool(on)
        for r in self._bwd_recs:
            if r[0] == "wreduce":
                r[1].accumulate = int(self.accumulate)

    def bwd_with_events(self, buckets, new_event):
        """Backward op list with SSDN_OP_EVENT_RECORD marks for the gradient exchange (ssdn.hip.dp).  buckets: list of sets of layer
        names; new_event(bucket indexes) -> raw hipEvent_t handle (int) that the all-reduce of those buckets will wait for.
        A bucket's slab reductions may run on SEVERAL lanes (plan "split": decode_block_2.2's on the side lane, the rest of its bucket
        on the main lane, and the executor orders no lane after another before the end-of-list join): the bucket gets one mark per
        lane, each on that lane right behind the bucket's last reduction THERE, and its collective waits for all of them
        (one mark on the lane of the last reduction in LIST order left the other lane's writes unordered).
        Marks that fall on the same (point of the list, lane) share one event."""
        lane_of = lambda r: r[2]                               # noqa: E731  (the scheduled lane)
        last = {}                                              # (bucket, lane) -> index of the bucket's last reduction on that lane
        for i, name in enumerate(self._bwd_layers):
            if name is None:
                continue
            for k, b in enumerate(buckets):
                if name in b:
                    last[(k, lane_of(self._bwd_recs[i]))] = i
        # (a mark inside a run of consecutive reductions of one lane would split the run -- the executor merges a run into two
        #  launches --: it moves to the end of the run; buckets that end in the same run are then marked at the same point)
        marks = {}                                             # (index, lane) -> buckets
        for (k, lane), i in last.items():
            while i + 1 < len(self._bwd_recs) and self._bwd_recs[i + 1][0] == "wreduce" and lane_of(self._bwd_recs[i + 1]) == lane:
                i += 1
            marks.setdefault((i, lane), []).append(k)
        recs, self.marks = [], []
        for i, r in enumerate(self._bwd_recs):
            recs.append(r)
            for (idx, lane), ks in sorted(marks.items()):
                if idx == i:
                    recs.append(("event_record", L.EventArgs(new_event(sorted(ks))), lane))
                    self.marks.append((len(recs) - 1, lane, sorted(ks)))
        ol = OpList(recs)
        # buckets whose LAST marks sit at the same point of the list complete together: the exchange may merge their collectives
        done_at = {}
        for (idx, lane), ks in marks.items():
            for k in ks:
                done_at[k] = max(done_at.get(k, -1), idx)
        by_pos = {}
        for k, idx in done_at.items():
            by_pos.setdefault(idx, []).append(k)
        ol.coincident = [sorted(ks) for _, ks in sorted(by_pos.items())]
        ol.marks = list(self.marks)
        return ol

    # ---- helpers ------------------------------------------------------------------------------------------
    def tensor(self, short: str) -> torch.Tensor:
        return self.t[self.plan.prefix + short]

    def _view(self, v: Optional[View]) -> L.View:
        if v is None:
            return L.View(None, 0, 0)
        t = self.t[v.t]
        return L.View(_ptr(t), t.shape[-1], v.co)

    def _pp(self, off_floats: int) -> int:
        return _ptr(self.params, 4 * (self.plan.param_base + off_floats))

    def _gp(self, off_floats: int) -> int:
        return _ptr(self.grads, 4 * (self.plan.param_base + off_floats))

    def _layer(self, name):
        return next(l for l in self.plan.layers if l.name == name)

    def _mat(self, op: Op):
        a = op.a
        P = self.plan.prefix
        if op.type == "pack_input":
            return op.type, L.PackInputArgs(_ptr(self.t[a["src"]]), self._view(a["dst"]), a["B"], a["C"], a["H"], a["W"], a["R"], a["cpad"])
        if op.type == "conv":
            l = self._layer(a["layer"])
            fwd = a["role"] == "fwd"

            def ptr(field, name):
                if field == "w":
                    return _ptr(self.t[P + ("wf/" if fwd else "wd/") + name])
                if field == "wc":      # the chunk-major copy, where the plan has one
                    wc = self.t.get(P + ("wfc/" if fwd else "wdc/") + name)
                    return _ptr(wc) if wc is not None else None
                if field == "bias":
                    return self._pp(l.b_off)
                return _ptr(self.t[name])
            s = L.conv_args(a, self._view, ptr)
            # the planner's rules against the library's (the planner restates them: ssdn/hip/graph.py)
            if a.get("pool") is not None and not L.load().ssdn_conv_fuses_pool(C.byref(s)):
                raise L.SsdnHipError("conv %s: the plan fuses the max-pool but the library cannot (planner / library rule mismatch)" % a["layer"])
            if a.get("upsum") is not None and not L.load().ssdn_conv_fuses_upsum(C.byref(s)):
                raise L.SsdnHipError("conv %s: the plan fuses UPSUM_BWD but the library cannot (planner / library rule mismatch)" % a["layer"])
            if (a.get("sign_out") or a.get("mask_sign") or a.get("upsum_mask_sign")) and not L.load().ssdn_conv_signs(C.byref(s)):
                raise L.SsdnHipError("conv %s: the plan uses sign bytes but the library cannot (planner / library rule mismatch)" % a["layer"])
            if a.get("urot") is not None and not L.load().ssdn_conv_fuses_urot(C.byref(s)):
                raise L.SsdnHipError("conv %s: the plan fuses UNROT_FWD but the library cannot (planner / library rule mismatch)" % a["layer"])
            if a.get("unrot") is not None and not L.load().ssdn_conv_fuses_unrot(C.byref(s)):
                raise L.SsdnHipError("conv %s: the plan fuses UNROT_BWD but the library cannot (planner / library rule mismatch)" % a["layer"])
            if L.load().ssdn_conv_lds_bytes(C.byref(s)) < 0:
                raise L.SsdnHipError("conv %s/%s: %s" % (a["layer"], a["role"], L.load().ssdn_last_error().decode()))
            return op.type, s
        if op.type in ("pool_fwd", "pool_bwd"):
            return op.type, L.PoolArgs(self._view(a["act"]), self._view(a.get("pooled")), self._view(a.get("dpool")),
                                       self._view(a.get("dz")), a["N"], a["H"], a["W"], a["C"], a["shifted"],
                                       self.t[a["route"]].data_ptr() if a.get("route") else None)
        if op.type == "upsum_bwd":
            return op.type, L.UpsumArgs(self._view(a["src"]), self._view(a["mask"]), self._view(a["dst"]), a["N"], a["H"], a["W"], a["C"])
        if op.type in ("unrot_fwd", "unrot_bwd"):
            return op.type, L.UnrotArgs(self._view(a["src"]), self._view(a["dst"]), self._view(a.get("mask")), a["B"], a["P"], a["C"],
                                        self.t[a["smask"]].data_ptr() if a.get("smask") else None)
        if op.type == "wgrad":
            s = L.WgradArgs()
            s.dz, s.src0, s.src1 = self._view(a["dz"]), self._view(a["src0"]), self._view(a["src1"])
            s.c0, s.c1, s.up0 = a["c0"], a["c1"], a["up0"]
            s.N, s.H, s.W = a["N"], a["H"], a["W"]
            s.ntaps = len(a["taps"])
            for i, (dy, dx) in enumerate(a["taps"]):
                s.dy[i], s.dx[i] = dy, dx
                s.coff[i] = a["coff"][i]
            s.M, s.Mpad, s.Ktot, s.Kpad = a["M"], a["Mpad"], a["Ktot"], a["Kpad"]
            s.slab, s.bslab = _ptr(self.t[a["slab"]]), _ptr(self.t[a["bslab"]])
            s.nslabs = a["nslabs"]
            s.ltw, s.lth, s.ltn = a["ltw"], a["lth"], a["ltn"]
            s.csplit = a.get("csplit", 0)
            s.mblocks = a.get("mblocks", 1)
            s.kreal = a.get("kreal", 0)
            s.mega, s.cost = a.get("mega", 0), a.get("cost", 0.0)
            if L.load().ssdn_wgrad_lds_bytes(C.byref(s)) < 0:
                raise L.SsdnHipError("wgrad %s: %s" % (a["layer"], L.load().ssdn_last_error().decode()))
            return op.type, s
        if op.type == "wreduce":
            l = self._layer(a["layer"])
            # (a merged weight-gradient launch owns mblocks consecutive groups of nslabs slabs: this reduction reads group mblock)
            mb = a.get("mblock", 0)
            soff = 4 * mb * a["nslabs"] * a["ntaps"] * a["Mpad"] * a["Kpad"]
            boff = 4 * mb * a["nslabs"] * a["Mpad"]
            return op.type, L.WreduceArgs(_ptr(self.t[a["slab"]], soff), _ptr(self.t[a["bslab"]], boff), a["nslabs"], a["ntaps"], a["M"],
                                          a["Mpad"], a["Kpad"], a["cin"], a["cin_full"], a["m_off"], a["c_off"], a["tapblock"],
                                          self._gp(l.w_off), self._gp(l.b_off) if a["with_bias"] else None,
                                          _ptr(self.t[P + "scale"], 4))
        if op.type == "wpack":
            l = self._layer(a["layer"])
            return op.type, L.WpackArgs(self._pp(l.w_off), _ptr(self.t[P + "wf/" + l.name]),
                                        _ptr(self.t[P + "wd/" + l.name]) if a["need_d"] else None, a["M"], a["cin"], a["ntaps"],
                                        a["c0"], a["c1_real"], a["Mpad_f"], a["Ktot"], a["Mpad_d"], a["Kd"],
                                        _ptr(self.t[P + "wfc/" + l.name]) if a.get("cm_f") else None,
                                        _ptr(self.t[P + "wdc/" + l.name]) if a.get("cm_d") else None)
        if op.type == "grad_pack":
            return op.type, L.GradPackArgs(_ptr(self.t[a["g"]]), self._view(a["dst"]), a["N"], a["C"], a["H"], a["W"], a["cpad"],
                                           _ptr(self.t[P + "gmax"]), _ptr(self.t[P + "scale"]))
        if op.type == "input_grad":
            s = L.InputGradArgs()
            s.g_e0, s.g_d1a = self._view(a["g_e0"]), self._view(a["g_d1a"])
            s.w_e, s.w_d = self._pp(self._layer(a["layer_e"]).w_off), self._pp(self._layer(a["layer_d"]).w_off)
            s.out = _ptr(self.t[a["dst"]])
            s.B, s.C, s.H, s.W, s.R = a["B"], a["C"], a["H"], a["W"], a["R"]
            s.ntaps = len(a["taps"])
            for i, (dy, dx) in enumerate(a["taps"]):
                s.dy[i], s.dx[i] = dy, dx
            return op.type, s
        raise ValueError("unknown op type " + op.type)


# Denoiser.train_step without a gradient exchange leaves the last bucket's slab reductions to the optimiser call (DeviceEngine.backward)
DEFER_TAIL = True
# Pixels of one sample a workgroup of the loss-head kernel walks (256 threads): 1024 = four pixels per thread in sequence.  (One pixel per
# thread used to be slower, 33 vs 20 us, because every WAVE ended with an atomic on the gradient sentinel; the kernel now issues one per block.)
HEAD_PX_PER_BLOCK = 1024

STYLE = {"gauss": 0, "poisson": 1, "impulse": 2}
MODE = {"known": 0, "const": 1, "var": 2}


def engine_style(style: str) -> str:
    """the head's noise model of a style string: impulse (csrc/head_impulse.hip; NOISE_STD_DEV carries alpha, one value per sample like
    gauss), poisson, and gauss for every other string, as ever"""
    return "poisson" if style.startswith("poisson") else "impulse" if style.startswith("impulse") else "gauss"


class DenoiserEngine:
    """Everything one Denoiser configuration needs on one GPU for one input shape: the main net, the optional sigma
    estimator, the loss head, the fused Adam pass -- as four op lists (fwd+loss, bwd, optimiser, eval)."""

    def __init__(self, pipeline: str, channels: int, blindspot: bool, style: str, mode: str, B: int, H: int, W: int,
                 device, params: torch.Tensor, grads: torch.Tensor, adam_m: torch.Tensor, adam_v: torch.Tensor,
                 n_main: int, n_sigma: int, has_est: bool, train: bool = True, ncoords: int = 64, input_grad: bool = False,
                 diag: bool = False):
        if input_grad and not train:
            raise ValueError("input_grad needs a training engine (train=True)")
        self.pipeline, self.C, self.blindspot, self.mode = pipeline, channels, blindspot, mode
        # DIAGONAL_COVARIANCE (ssdn): the network's 2*C outputs are the means and the diagonal of A
        self.diag = bool(diag) and pipeline == "ssdn"
        self.input_grad = bool(input_grad)
        self.style = engine_style(style)
        if self.style == "impulse" and self.diag:
            raise NotImplementedError("DIAGONAL_COVARIANCE is not implemented for the impulse noise model")
        self.B, self.H, self.W, self.device, self.train = B, H, W, device, train
        self.params, self.grads, self.m, self.v = params, grads, adam_m, adam_v
        lib = L.load()
        cus = lib.ssdn_device_cus()
        if cus <= 0:
            raise L.SsdnHipError("no HIP device: " + lib.ssdn_last_error().decode())
        cout = (2 * channels if self.diag else channels + channels * (channels + 1) // 2) if pipeline == "ssdn" else channels
        f32 = dict(dtype=torch.float32, device=device)
        self.inp = torch.zeros((B, channels, H, W), **f32)
        var = pipeline == "ssdn" and mode == "var"
        self.main = DeviceNet(NetPlan("m/", channels, cout, blindspot, B, H, W, cus=cus, train=train, param_base=0, input_grad=self.input_grad),
                              device, params, grads, shared={"m/in32": self.inp}, hold_input_grad=self.input_grad and var)
        self.sigma = None
        if var:
            self.sigma = DeviceNet(NetPlan("s/", channels, 1, False, B, H, W, cus=cus, train=train, param_base=n_main, input_grad=self.input_grad),
                                   device, params, grads, shared={"s/in32": self.inp})
        # dL/d(noisy input) of the autograd route (vjp_backward(want_dx=True)), summed on the device in ONE fixed order:
        #   dx = S_main + (S_sigma + head)
        # head: the loss head's direct term (SSDN_OP_HEAD_VJP's g_noisy, written first); S_sigma / S_main: the two networks'
        # SSDN_OP_INPUT_GRAD sums, each adding the term before it last.  The main network's op writes `dx` in place (add = out = dx)
        # inside its backward list; in mode var the sigma network's runs on the side stream into its own dx32 (add = dx) and the main
        # network's is held out of its list and enqueued behind the join (add = the sigma network's dx32).  MSE pipelines: dx = S_main.
        # (a backward pass without the head term -- Denoiser.backward(), vjp_backward without want_dx -- leaves the head's addend off:
        #  `dx` then holds the networks' terms only, and never accumulates across passes)
        self.dx = None
        if self.input_grad:
            self.dx = self.main.tensor("dx32")
            if self.sigma is not None:
                self.main.input_grad_args.add = _ptr(self.sigma.tensor("dx32"))
        self.est_off = n_main + n_sigma if has_est else None
        # loss-side buffers
        self.loss = torch.zeros((B, 1), **f32)
        self.ref = torch.zeros((B, channels, H, W), **f32)
        self.noise_param = torch.zeros((B,), **f32)
        self.coords = torch.zeros((ncoords, 2), dtype=torch.int64, device=device)
        self.ncoords = ncoords
        self.nchunks = max(1, min(64, (H * W) // HEAD_PX_PER_BLOCK))
        self.partial = torch.zeros((B, self.nchunks, 2), **f32)
        self.est_raw = torch.zeros((B,), **f32)
        self.g_est_var = torch.zeros((B,), **f32)
        self.mu = torch.zeros((B, channels, H, W), **f32)
        self.pme = torch.zeros((B, channels, H, W), **f32)
        self.model_std = torch.zeros((B, H, W), **f32)
        self.noise_std = torch.zeros((B, H, W) if self.style == "poisson" else (B,), **f32)
        self.zero_buf = torch.zeros((8,), dtype=torch.int32, device=device)   # unused gmax sink for eval
        self._adam_args = None
        # gradient accumulation (set_accumulate): a pass that ADDS to the flat gradient.  The learnable noise scalar of mode const has no
        # slab reduction: SSDN_OP_HEAD_FINAL (in the FORWARD list) and SSDN_OP_HEAD_VJP store its gradient, so in an accumulating pass
        # they store into this staging float and the backward pass folds it into the running sum with one SSDN_OP_ACCUM launch.
        self.accumulate = False
        self.stages_est = bool(train and pipeline == "ssdn" and mode == "const" and self.est_off is not None)
        self.g_est_stage = torch.zeros((1,), **f32) if self.stages_est else None
        self._head_final_args = None
        self._accum_ops = None
        # H11: loss / PSNR / std-dev sums of a step go into a device-resident accumulator (SSDN_OP_METRICS); `per` holds the last
        # batch's per-sample values (the evaluator's per-image PSNR)
        self.metrics_per = torch.zeros((B, 8), **f32)
        self._metrics_args = None
        self.ops_loss = OpList(self._loss_ops(want_grad=train))
        opt_recs = self._opt_ops() if train else None          # (both lists share the argument structs adam() updates)
        self.ops_opt = OpList(opt_recs) if train else None
        self.ops_opt_tail = OpList(self.main.tail_recs + opt_recs) if train and self.main.tail_recs else None
        self._tail_pending = False
        # autograd route (Denoiser.run_pipeline): generation = training forwards so far (a graph of an older one cannot backward);
        # g_fresh: g32 / the partials still hold what the forward's loss op wrote (d mean(LOSS)), not a vector-Jacobian product's
        self.gen = 0
        self.g_fresh = self.loss_fwd = False
        self._vjp = None
        self._post = {}             # posterior(): cov / std / samples buffers, allocated on first use (no plan tensor)
        self._ssim = {}             # ssim(): value / map / scratch buffers, allocated on first use (no plan tensor)
        self._calib = {}            # calibration(): stats / hist / zmap / scratch buffers, allocated on first use (no plan tensor)
        self._risk = {}             # risk(): stats / scratch buffers, allocated on first use (no plan tensor)
        self._img = {}              # image_in() / image_out() / estimate_noise(): pinned and device byte buffers with their tables, allocated on first use (no plan tensor)

    # ---- op construction -----------------------------------------------------------------------------------
    def _gmax(self, net: Optional[DeviceNet]):
        if net is not None and self.train:
            return _ptr(net.tensor("gmax"))
        return _ptr(self.zero_buf)

    def _loss_ops(self, want_grad: bool):
        recs = []
        B, Cn, H, W = self.B, self.C, self.H, self.W
        out32 = self.main.tensor("out32")
        g32 = _ptr(self.main.tensor("g32")) if want_grad else None
        # (gmax, the max-|gradient| sentinel the loss kernels fold into with atomicMax, is a RUNNING maximum since the buffers were created:
        #  clearing its 16 bytes every step was a launch of its own in the serial stretch between the forward and the backward pass)
        if self.pipeline == "ssdn":
            est_ptr = None
            if self.mode == "var":
                recs.append(("spatial_mean", L.SpatialMeanArgs(_ptr(self.sigma.tensor("out32")), _ptr(self.est_raw), B, H * W)))
                est_ptr = _ptr(self.est_raw)
            elif self.mode == "const":
                est_ptr = _ptr(self.params, 4 * self.est_off)
            recs.append(("head_ssdn", L.HeadArgs(_ptr(out32), _ptr(self.inp), _ptr(self.noise_param), est_ptr, B, Cn, H, W,
                                                  STYLE[self.style], MODE[self.mode], int(want_grad), _ptr(self.mu), _ptr(self.pme),
                                                  _ptr(self.model_std), _ptr(self.noise_std), g32, _ptr(self.partial),
                                                  self.nchunks, self._gmax(self.main), int(self.diag))))
            g_est = self._g_est_ptr() if want_grad else None
            recs.append(("head_final", L.HeadFinalArgs(_ptr(self.partial), B, self.nchunks, H, W, MODE[self.mode], _ptr(self.loss), g_est,
                                                        _ptr(self.sigma.tensor("g32")) if (want_grad and self.sigma is not None) else None,
                                                        self._gmax(self.sigma) if self.sigma is not None else None)))
            self._head_final_args = recs[-1][1]
        elif self.pipeline == "mse":
            recs.append(("mse", L.MseArgs(_ptr(out32), _ptr(self.ref), None, 0, B, Cn, H, W, _ptr(self.loss), g32, self._gmax(self.main))))
        elif self.pipeline == "mask_mse":
            recs.append(("mask_mse", L.MseArgs(_ptr(out32), _ptr(self.ref), _ptr(self.coords), self.ncoords, B, Cn, H, W, _ptr(self.loss),
                                               g32, self._gmax(self.main))))
        else:
            raise NotImplementedError("Unsupported processing pipeline")
        return recs

    def _g_est_ptr(self):
        """where the head ops store the gradient of the noise estimate: const: the flat gradient's last element, or the staging float in
        an accumulating pass; var: the per-sample buffer (per pass either way); known: nowhere"""
        if self.mode == "const":
            return _ptr(self.g_est_stage) if self.accumulate and self.stages_est else _ptr(self.grads, 4 * self.est_off)
        if self.mode == "var":
            return _ptr(self.g_est_var)
        return None

    def set_accumulate(self, on: bool) -> None:
        """The passes from the next FORWARD on add their parameter gradients to the flat gradient buffer (on) or overwrite it (off, the
        default).  Decided before the forward is enqueued: in mode const the forward's loss op already stores the noise scalar's
        gradient.  Idempotent; mutates argument structs in place, rebuilds no list."""
        on = bool(on)
        if on == self.accumulate:
            return
        if on and not self.train:
            raise L.SsdnHipError("set_accumulate needs a training engine")
        self.accumulate = on
        self.main.set_accumulate(on)
        if self.sigma is not None:
            self.sigma.set_accumulate(on)
        if self.stages_est:
            if self._head_final_args is not None and self._head_final_args.g_est:
                self._head_final_args.g_est = self._g_est_ptr()
            if self._vjp is not None:
                self._vjp[0].g_est = self._g_est_ptr()
            if on and self._accum_ops is None:
                self._accum_ops = OpList([("accum", L.AccumArgs(_ptr(self.grads, 4 * self.est_off), _ptr(self.g_est_stage), 1))])

    def _opt_ops(self):
        """Fused Adam over the flat buffer, each range directly followed by the re-packs of the layers inside it: the executor
        runs such a run as ONE launch (k_adam_pack: the thread that updates a weight also writes its fp16 / bf16 shadows)."""
        def adam(lo, hi):
            return L.AdamArgs(_ptr(self.params, 4 * lo), _ptr(self.grads, 4 * lo), _ptr(self.m, 4 * lo), _ptr(self.v, 4 * lo), hi - lo,
                              0.0, 0.9, 0.99, 1e-8, 1.0, 1.0, 1.0)
        n_tot = self.params.numel()
        n_main = self.sigma.plan.param_base if self.sigma is not None else n_tot
        self._adam_args = [adam(0, n_main)]
        recs = [("adam", self._adam_args[0])] + [self.main._mat(op) for op in self.main.plan.pack]
        if self.sigma is not None:
            self._adam_args.append(adam(n_main, n_tot))
            recs += [("adam", self._adam_args[1])] + [self.sigma._mat(op) for op in self.sigma.plan.pack]
        return recs

    # ---- metrics (H11) -------------------------------------------------------------------------------------
    def accumulate_metrics(self, acc: torch.Tensor, clean: Optional[torch.Tensor], ext: Optional[torch.Tensor] = None, with_loss: bool = True,
                           stream=None):
        """Enqueue ONE launch that adds this batch's loss / PSNR(out) / PSNR(mu) / noise std / model std sums into `acc` (fp32 [16] on
        the device: sum, count per metric) -- the reference's per-step `Metric +=` lines (train.py:205-218).  clean: fp32 [B,C,H,W] on
        the device; ext: int32 [B,2] valid extents of the two spatial axes (padded evaluation images) or None.
        clean=None (a batch of images that are already noisy: there is no clean image): the kernel skips a metric whose source pointer is
        null, so the two image outputs are withheld and no PSNR sum or count moves; `clean` is then any valid buffer, the engine's input."""
        a = self._metrics_args
        if a is None:
            a = self._metrics_args = L.MetricsArgs()
            a.B, a.C, a.H, a.W = self.B, self.C, self.H, self.W
            a.per = _ptr(self.metrics_per)
            if self.pipeline == "ssdn":
                a.model_std, a.noise_std = _ptr(self.model_std), _ptr(self.noise_std)
                # (gauss, impulse: one value per sample -- one for the whole batch when it is a learnt constant; poisson: per pixel)
                a.noise_n = self.noise_std.numel() if self.style == "poisson" else (1 if self.mode == "const" else self.B)
            self._metrics_ops = OpList([("metrics", a)])
        if clean is None:
            a.out, a.mu, clean = None, None, self.inp
        elif self.pipeline == "ssdn":
            a.out, a.mu = _ptr(self.pme), _ptr(self.mu)
        else:
            a.out = _ptr(self.main.tensor("out32"))
        if clean.dtype != torch.float32 or not clean.is_contiguous() or tuple(clean.shape) != (self.B, self.C, self.H, self.W):
            raise L.SsdnHipError("metrics: clean must be a contiguous fp32 [B,C,H,W] device tensor of the engine's shape")
        a.clean, a.acc = _ptr(clean), _ptr(acc)
        a.loss = _ptr(self.loss) if with_loss else None
        a.ext = _ptr(ext) if ext is not None else None
        self._metrics_ops.run(current_stream() if stream is None else stream)

    # ---- export: the whole step as a blob libssdn_hip.so runs on its own (csrc/plan.hip, include/ssdn_hip.h "step-level entry points") ----
    def export_plan(self, meta: Optional[dict] = None) -> bytes:
        """The op lists of this engine with every pointer replaced by (tensor, offset), the tensor table, and a JSON description.
        ssdn_plan_load() + ssdn_plan_bind() rebuild them in one caller-owned arena; ssdn_train_step() / ssdn_net_forward() run them --
        a binder needs the library and this blob, not the Python package."""
        if self.input_grad:
            raise L.SsdnHipError("export_plan: input-gradient engines (the autograd route's) are not part of the plan blob")
        if self.accumulate:          # a blob always holds overwriting passes (accumulate = 0, g_est in the flat gradient)
            self.set_accumulate(False)
            try:
                return self.export_plan(meta)
            finally:
                self.set_accumulate(True)
        import json
        import struct
        tens: List[tuple] = []                       # (name, tensor)
        for name, t in self.main.t.items():
            tens.append((name, t))
        if self.sigma is not None:
            for name, t in self.sigma.t.items():
                tens.append((name, t))
        tens += [("params", self.params), ("grads", self.grads), ("adam_m", self.m), ("adam_v", self.v), ("loss", self.loss), ("ref", self.ref),
                 ("noise_param", self.noise_param), ("coords", self.coords), ("partial", self.partial), ("est_raw", self.est_raw),
                 ("g_est_var", self.g_est_var), ("mu", self.mu), ("pme", self.pme), ("model_std", self.model_std), ("noise_std", self.noise_std),
                 ("zero_buf", self.zero_buf), ("metrics_per", self.metrics_per)]
        tens = [(n, t) for n, t in tens if t is not None]
        table, by_ptr = [], {}
        for name, t in tens:
            nbytes = t.numel() * t.element_size()
            ptr = t.data_ptr()
            alias = by_ptr.get(ptr, -1)
            if alias >= 0 and table[alias][1] < nbytes:
                raise L.SsdnHipError("export_plan: tensor %s aliases a smaller one" % name)
            if alias < 0:
                by_ptr[ptr] = len(table)
            table.append((name, nbytes, alias, ptr))
        spans = sorted((ptr, ptr + nb, i) for i, (n, nb, al, ptr) in enumerate(table) if al < 0)

        def locate(v):
            for lo, hi, i in spans:
                if lo <= v < hi or (v == hi == lo):
                    return i, v - lo
            raise L.SsdnHipError("export_plan: an op argument points outside every tensor of the engine (0x%x)" % v)
        ptr_off = {ty: L.pointer_fields(ty) for ty in set(L.ARG_TYPES.values())}

        def ser(oplists):
            out, n = b"", 0
            for ol in oplists:
                if ol is None:
                    continue
                for i in range(ol.n):
                    a = ol.args[i]
                    raw = bytes(a)
                    rel = b""
                    nr = 0
                    for off in ptr_off[type(a)]:
                        v = struct.unpack_from("<Q", raw, off)[0]
                        if v:
                            ti, d = locate(v)
                            rel += struct.pack("<IIQ", off, ti, d)
                            nr += 1
                    pad = (-len(raw)) % 8
                    out += struct.pack("<iiII", int(ol.arr[i].type), int(ol.arr[i].lane), len(raw), nr) + raw + b"\0" * pad + rel
                    n += 1
            return struct.pack("<I", n) + out
        train = self.train
        phases = [[self.main.pack, self.sigma.pack if self.sigma is not None else None],
                  [self.main.fwd, self.sigma.fwd if self.sigma is not None else None, self.ops_loss],
                  [self.main.bwd, self.sigma.bwd if self.sigma is not None else None] if train else [],
                  [self.ops_opt] if train else []]
        layers = lambda net, base: [dict(name=l.name, w_off=base + l.w_off, b_off=base + l.b_off, M=l.M, cin=l.cin, k=l.k) for l in net.plan.layers]   # noqa: E731
        desc = dict(pipeline=self.pipeline, channels=self.C, blindspot=bool(self.blindspot), style=self.style, mode=self.mode, diag=self.diag, B=self.B, H=self.H,
                    W=self.W, train=bool(train), nparams=int(self.params.numel()), est_off=self.est_off,
                    layers=layers(self.main, 0) + (layers(self.sigma, self.sigma.plan.param_base) if self.sigma is not None else []))
        desc.update(meta or {})
        mj = json.dumps(desc).encode()
        blob = b"SSDNPLAN" + struct.pack("<IIII", 1, L.ABI_VERSION, len(table), 4)
        for name, nb, al, _ in table:
            nm = name.encode()
            if len(nm) > 55:
                raise L.SsdnHipError("export_plan: tensor name too long: " + name)
            blob += nm + b"\0" * (56 - len(nm)) + struct.pack("<Qii", nb, al, 0)
        for ph in phases:
            blob += ser(ph)
        return blob + struct.pack("<I", len(mj)) + mj

    # ---- execution -----------------------------------------------------------------------------------------
    def repack(self, stream=None):
        s = current_stream() if stream is None else stream
        self.main.pack.run(s)
        if self.sigma is not None:
            self.sigma.pack.run(s)

    # ---- the sigma-estimation network next to the main network (BASELINE config 3) ------------------------------------------------
    # The two networks share only the input and meet in the loss head (reference: ssdn/ssdn/denoiser.py:76-88, 261-265: the estimator
    # reads the noisy image, nothing of the main network).  Enqueued one behind the other on ONE stream (rounds 1-5) the small plain
    # network -- grids of a few dozen workgroups at batch 32 -- ran alone on the chip for 0.86 ms of a 2.5 ms step.  Now its op lists go
    # to a second stream, ordered behind what the caller's stream has enqueued so far and joined back before the consumer (loss head /
    # optimiser): its launches fill the CUs the main network's latency-bound stages leave idle.  Every tensor the two lists write is its
    # own (each DeviceNet owns its buffers; disjoint ranges of the flat gradient), so the results are the sequential order's, bit for bit.
    SIGMA_CONCURRENT = 3          # bit 0: forward lists, bit 1: backward lists (True = both)

    def _fork_sigma(self, s: int, oplist) -> int:
        """run `oplist` (the sigma network's) on the side stream behind everything stream `s` holds; -> the side stream (to join on)"""
        if getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream(device=self.device)
        side = self._side.cuda_stream
        # (the library's own event ring on the RAW handles.  The first version recorded a torch.cuda.Event on torch.cuda.ExternalStream(s) with
        #  s = current_stream().cuda_stream: that wrapper of handle 0 is not ordered behind torch's current stream -- the side stream started
        #  early in ~5 of 12 runs (stale upstream gradients); an event recorded on the torch.cuda.current_stream() OBJECT orders correctly,
        #  12 of 12 (tools/ab_sigma_race.py, profiles/r06_sigma_concurrency.txt).  The engine is handed raw handles, so it orders raw handles.)
        L.check(L.load().ssdn_stream_order(C.c_void_p(s), C.c_void_p(side)))
        oplist.run(side)
        return side

    def _join_sigma(self, s: int, side: int) -> None:
        L.check(L.load().ssdn_stream_order(C.c_void_p(side), C.c_void_p(s)))

    def forward(self, stream=None):
        s = current_stream() if stream is None else stream
        if self.train:
            self.gen += 1
            self.g_fresh = self.loss_fwd = True
        if self.sigma is not None and (int(self.SIGMA_CONCURRENT) & 1):
            ev = self._fork_sigma(s, self.sigma.fwd)
            self.main.fwd.run(s)
            self._join_sigma(s, ev)
        else:
            self.main.fwd.run(s)
            if self.sigma is not None:
                self.sigma.fwd.run(s)
        self.ops_loss.run(s)

    def net_forward_only(self, stream=None):
        s = current_stream() if stream is None else stream
        if self.train:
            self.gen += 1
            self.g_fresh = self.loss_fwd = False
        self.main.fwd.run(s)

    def posterior(self, n_samples: int = 0, seed: int = 0, offset: int = 0, cov: bool = True, std: bool = True, stream=None):
        """The per-pixel posterior of the LAST forward beyond its mean (SSDN_OP_HEAD_POSTERIOR, csrc/head_posterior.hip): one launch on the
        engine's stream behind that forward, reading its net_out, input and noise estimate.  -> dict of "cov" [B, C(C+1)/2, H, W], "std"
        [B,C,H,W] and, for n_samples > 0, "samples" [n_samples, B, C, H, W]: the engine's own buffers, allocated on first use outside the
        plan's tensors and overwritten by the next call (an exported plan knows nothing of them).  Nothing here is differentiable."""
        if self.pipeline != "ssdn":
            raise NotImplementedError("the posterior covariance exists for the ssdn pipeline only")
        n_samples = int(n_samples)
        if n_samples < 0:
            raise ValueError("n_samples must be >= 0")
        if not (cov or std or n_samples):
            raise ValueError("posterior: nothing requested")
        B, Cn, H, W = self.B, self.C, self.H, self.W
        f32 = dict(dtype=torch.float32, device=self.device)
        buf = self._post
        if cov and "cov" not in buf:
            buf["cov"] = torch.zeros((B, Cn * (Cn + 1) // 2, H, W), **f32)
        if std and "std" not in buf:
            buf["std"] = torch.zeros((B, Cn, H, W), **f32)
        if n_samples and ("samples" not in buf or buf["samples"].shape[0] != n_samples):
            buf["samples"] = torch.zeros((n_samples, B, Cn, H, W), **f32)
        if self.mode == "var":
            est_ptr = _ptr(self.est_raw)
        else:
            est_ptr = _ptr(self.params, 4 * self.est_off) if self.mode == "const" else None
        a = L.HeadPosteriorArgs(_ptr(self.main.tensor("out32")), _ptr(self.inp), _ptr(self.noise_param), est_ptr, B, Cn, H, W,
                                STYLE[self.style], MODE[self.mode], int(self.diag), self.nchunks,
                                _ptr(buf["cov"]) if cov else None, _ptr(buf["std"]) if std else None,
                                _ptr(buf["samples"]) if n_samples else None, n_samples, int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1))
        OpList([("head_posterior", a)]).run(current_stream() if stream is None else stream)
        return {k: buf[k] for k, on in (("cov", cov), ("std", std), ("samples", n_samples > 0)) if on}

    def ssim(self, x: torch.Tensor, clean: torch.Tensor, ext: Optional[torch.Tensor] = None, want_map: bool = False, stream=None):
        """SSIM of `x` against `clean` (SSDN_OP_SSIM, csrc/ssim.hip) per sample over its un-padded extent: two launches on the engine's
        stream behind the last forward.  x, clean: contiguous fp32 [B,C,H,W] device tensors of the engine's shape (x is normally one of
        the engine's own: inp, pme, mu, the network output); ext: int32 [B,2] device tensor or None, accumulate_metrics' convention.
        -> (ssim [B], map [B,C,H,W] or None): the engine's own buffers, allocated on first use outside the plan's tensors and
        overwritten by the next call.  The map is zero where no window is centred."""
        shape = (self.B, self.C, self.H, self.W)
        for name, t in (("x", x), ("clean", clean)):
            if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape or t.device != self.inp.device:
                raise L.SsdnHipError("ssim: %s must be a contiguous fp32 [B,C,H,W] device tensor of the engine's shape" % name)
        f32 = dict(dtype=torch.float32, device=self.device)
        buf = self._ssim
        if "val" not in buf:
            buf["val"] = torch.zeros((self.B,), **f32)
            buf["scratch"] = torch.zeros((L.ssim_scratch_bytes(*shape) // 8,), dtype=torch.float64, device=self.device)
        if want_map:
            if "map" not in buf:
                buf["map"] = torch.zeros(shape, **f32)
            else:
                buf["map"].zero_()
        a = L.SsimArgs(_ptr(x), _ptr(clean), _ptr(ext) if ext is not None else None, *shape, _ptr(buf["val"]),
                       _ptr(buf["map"]) if want_map else None, _ptr(buf["scratch"]), buf["scratch"].numel() * 8)
        OpList([("ssim", a)]).run(current_stream() if stream is None else stream)
        return buf["val"], (buf["map"] if want_map else None)

    def calibration(self, clean: torch.Tensor, ext: Optional[torch.Tensor] = None, want_hist: bool = False, want_map: bool = False, stream=None):
        """Calibration statistics of the LAST forward's posterior N(pme, cov) against `clean` (SSDN_OP_CALIBRATION, csrc/calibration.hip)
        per sample over its un-padded extent: one posterior(cov=True, std=False) launch behind that forward, then the calibration op on
        self.pme, that cov buffer and clean.  clean: contiguous fp32 [B,C,H,W] device tensor of the engine's shape; ext: int32 [B,2] device
        tensor or None, accumulate_metrics' convention.  -> (stats [B,12] float64, hist [B,C,34] int64 or None, zmap [B,C,H,W] or None): the
        engine's own buffers, allocated on first use outside the plan's tensors and overwritten by the next call.  The map is NaN outside
        the extents."""
        shape = (self.B, self.C, self.H, self.W)
        if clean.dtype != torch.float32 or not clean.is_contiguous() or tuple(clean.shape) != shape or clean.device != self.inp.device:
            raise L.SsdnHipError("calibration: clean must be a contiguous fp32 [B,C,H,W] device tensor of the engine's shape")
        s = current_stream() if stream is None else stream
        cov = self.posterior(cov=True, std=False, stream=s)["cov"]
        buf = self._calib
        if "stats" not in buf:
            buf["stats"] = torch.zeros((self.B, L.CALIB_NSTATS), dtype=torch.float64, device=self.device)
            buf["scratch"] = torch.zeros((L.calib_scratch_bytes(*shape) // 8,), dtype=torch.float64, device=self.device)
        if want_hist and "hist" not in buf:
            buf["hist"] = torch.zeros((self.B, self.C, L.CALIB_HIST_BINS), dtype=torch.int64, device=self.device)
        if want_map:
            if "zmap" not in buf:
                buf["zmap"] = torch.empty(shape, dtype=torch.float32, device=self.device)
            buf["zmap"].fill_(float("nan"))
        a = L.CalibrationArgs(_ptr(self.pme), _ptr(cov), _ptr(clean), _ptr(ext) if ext is not None else None, *shape, _ptr(buf["stats"]),
                              _ptr(buf["hist"]) if want_hist else None, _ptr(buf["zmap"]) if want_map else None,
                              _ptr(buf["scratch"]), buf["scratch"].numel() * 8)
        OpList([("calibration", a)]).run(s)
        return buf["stats"], (buf["hist"] if want_hist else None), (buf["zmap"] if want_map else None)

    def risk(self, ext: Optional[torch.Tensor] = None, margin: int = 0, stream=None):
        """Reference-free risk statistics of the LAST forward (SSDN_OP_RISK, csrc/risk.hip) per sample over its margin-shrunk un-padded
        extent: two launches on the engine's stream behind that forward, reading its net_out, input, noise parameter / estimate and
        self.pme -- no clean image.  ext: int32 [B,2] device tensor or None, accumulate_metrics' convention.  -> stats [B,12] float64
        (ssdn.utils.risk_values derives the reported values): the engine's own buffer, allocated on first use outside the plan's tensors
        and overwritten by the next call.  Nothing is synchronised."""
        if self.pipeline != "ssdn":
            raise NotImplementedError("the risk estimate exists for the ssdn pipeline only")
        if self.style not in ("gauss", "poisson"):
            raise NotImplementedError("the risk estimate needs a gauss or poisson model: the %s posterior mean is not affine in the pixel "
                                      "and its noise is not zero-mean" % self.style)
        shape = (self.B, self.C, self.H, self.W)
        buf = self._risk
        if "stats" not in buf:
            buf["stats"] = torch.zeros((self.B, L.RISK_NSTATS), dtype=torch.float64, device=self.device)
            buf["scratch"] = torch.zeros((L.risk_scratch_bytes(*shape) // 8,), dtype=torch.float64, device=self.device)
        if self.mode == "var":
            est_ptr = _ptr(self.est_raw)
        else:
            est_ptr = _ptr(self.params, 4 * self.est_off) if self.mode == "const" else None
        a = L.RiskArgs(_ptr(self.main.tensor("out32")), _ptr(self.inp), _ptr(self.noise_param), est_ptr, _ptr(self.pme),
                       _ptr(ext) if ext is not None else None, *shape, STYLE[self.style], MODE[self.mode], int(self.diag), int(margin),
                       _ptr(buf["stats"]), _ptr(buf["scratch"]), buf["scratch"].numel() * 8)
        OpList([("risk", a)]).run(current_stream() if stream is None else stream)
        return buf["stats"]

    IMAGE_ALIGN = 16            # image_in(): every image of a batch starts on a multiple of this in the packed byte buffer

    def _image_buffers(self, bits: int = 8):
        """The buffers of image_in() / image_out(), sized for a full batch of un-padded images of the engine's shape: [offs: B int64 |
        ext: B x 2 int32 | the packed images], once pinned on the host and once on the device (one upload carries the tables and the
        samples), and the same pair for the images coming out.  Byte tensors per sample depth, allocated on the first batch of that depth
        (the uint16 batches' under the keys + "16"): the same head of tables, then the packed samples, every image on a multiple of
        IMAGE_ALIGN samples; uint16 samples are a view behind the head."""
        buf, k = self._img, "16" if bits == 16 else ""
        if "dev_in" + k not in buf:
            a = self.IMAGE_ALIGN
            buf["head"] = (16 * self.B + a - 1) // a * a
            n = buf["head"] + bits // 8 * self.B * ((self.C * self.H * self.W + a - 1) // a * a)
            buf["host_in" + k] = torch.zeros((n,), dtype=torch.uint8).pin_memory()
            buf["host_out" + k] = torch.zeros((n,), dtype=torch.uint8).pin_memory()
            buf["dev_in" + k] = torch.zeros((n,), dtype=torch.uint8, device=self.device)
            buf["dev_out" + k] = torch.zeros((n,), dtype=torch.uint8, device=self.device)
        return buf

    def image_in(self, images: List[torch.Tensor], white: Optional[int] = None) -> torch.Tensor:
        """Fill `self.inp` with a batch of whole images (SSDN_OP_IMAGE_IN, csrc/image_io.hip): one pinned upload of the packed bytes and
        their tables, one launch that divides by 255, transposes to the package's swapped axes and reflection-pads every image bottom
        and right to the engine's shape.  images: exactly B contiguous uint8 CPU tensors [h, w, C] (upright, as PIL hands them out) with
        w <= H and h <= W of the engine (tensor axis 2 runs along x).  -> self.inp, which `Denoiser._run` then takes without a copy.
        The tables stay on the device for the image_out() that follows.
        A batch of uint16 tensors runs SSDN_OP_IMAGE_IN16 (the same kernel over uint16 samples; offsets and counts are then in samples):
        two bytes per sample cross the bus, the value is min(sample, white) / white with `white` the sample value that means 1.0
        (default 65535; refused for bytes), and image_out() then returns uint16 at the same white level.  A batch is of one dtype."""
        B, Cn = self.B, self.C
        if len(images) != B:
            raise L.SsdnHipError("image_in: %d images for an engine of batch %d" % (len(images), B))
        wide = images[0].dtype == torch.uint16
        if wide:
            white = check_white(white)
        elif white is not None:
            raise L.SsdnHipError("image_in: white is for uint16 images")
        bits, k, dtype = (16, "16", torch.uint16) if wide else (8, "", torch.uint8)
        for t in images:
            if (t.dtype != dtype or t.device.type != "cpu" or t.dim() != 3 or t.shape[2] != Cn or not t.is_contiguous()
                    or not (1 <= t.shape[1] <= self.H and 1 <= t.shape[0] <= self.W)):
                raise L.SsdnHipError(("image_in: every image of a uint16 batch must be a contiguous uint16 CPU tensor [h, w, %d] with "
                                      "w <= %d and h <= %d" if wide else
                                      "image_in: every image must be a contiguous uint8 CPU tensor [h, w, %d] with w <= %d and h <= %d")
                                     % (Cn, self.H, self.W))
        buf = self._image_buffers(bits)
        host, a, head = buf["host_in" + k], self.IMAGE_ALIGN, buf["head"]
        samples = host[head:].view(dtype)
        offs, pos = [], 0
        for t in images:
            offs.append(pos)
            samples[pos:pos + t.numel()] = t.reshape(-1)
            pos += (t.numel() + a - 1) // a * a
        host[:8 * B].view(torch.int64).copy_(torch.tensor(offs, dtype=torch.int64))
        host[8 * B:16 * B].view(torch.int32).copy_(torch.tensor([[t.shape[1], t.shape[0]] for t in images], dtype=torch.int32).reshape(-1))
        n = head + bits // 8 * pos
        dev = buf["dev_in" + k]
        dev[:n].copy_(host[:n], non_blocking=True)
        buf["offs"], buf["shapes"], buf["bytes"], buf["bits"], buf["white"] = offs, [tuple(t.shape) for t in images], pos, bits, white
        batch = (_ptr(dev, head), pos, _ptr(dev), _ptr(dev, 8 * B), B, Cn, self.H, self.W)
        if wide:
            rec = ("image_in16", L.ImageIn16Args(*batch, white, _ptr(self.inp)))
        else:
            rec = ("image_in", L.ImageInArgs(*batch, _ptr(self.inp)))
        OpList([rec]).run(current_stream())                      # (behind the upload, on torch's current stream)
        return self.inp

    def image_out(self, x: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
        """The images of the last image_in() batch out of `x` (default: the denoised batch -- self.pme, the network output for the MSE
        pipelines) as bytes (SSDN_OP_IMAGE_OUT): one launch that crops to every extent, clips to [0, 1], multiplies by 255, truncates
        and transposes back, one download.  -> B uint8 CPU tensors [h, w, C]: views of the engine's pinned buffer, overwritten by the
        next call.  Synchronises.  After a uint16 image_in(): SSDN_OP_IMAGE_OUT16 -- clip, * white, round to nearest even -- and uint16
        tensors, at that batch's white level."""
        buf = self._img
        if "offs" not in buf:
            raise L.SsdnHipError("image_out: needs a preceding image_in()")
        if x is None:
            x = self.pme if self.pipeline == "ssdn" else self.main.tensor("out32")
        shape = (self.B, self.C, self.H, self.W)
        if x.dtype != torch.float32 or not x.is_contiguous() or tuple(x.shape) != shape or x.device != self.inp.device:
            raise L.SsdnHipError("image_out: x must be a contiguous fp32 [B,C,H,W] device tensor of the engine's shape")
        wide = buf["bits"] == 16
        k, size = ("16", 2) if wide else ("", 1)
        dev, dev_out, host, n = buf["dev_in" + k], buf["dev_out" + k], buf["host_out" + k], buf["bytes"]
        batch = (_ptr(x), _ptr(dev, 8 * self.B), _ptr(dev), _ptr(dev_out), n, *shape)
        rec = ("image_out16", L.ImageOut16Args(*batch, buf["white"])) if wide else ("image_out", L.ImageOutArgs(*batch))
        OpList([rec]).run(current_stream())
        host[:size * n].copy_(dev_out[:size * n], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        out = host.view(torch.uint16) if wide else host
        return [out[o:o + h * w * c].view(h, w, c) for o, (h, w, c) in zip(buf["offs"], buf["shapes"])]

    def image_extents(self) -> torch.Tensor:
        """The un-padded extents (w_b, h_b) of the last image_in() batch as the ops read them: an int32 [B,2] view of the table that batch
        left on the device (SSDN_OP_METRICS' convention)."""
        buf = self._img
        if "offs" not in buf:
            raise L.SsdnHipError("image_extents: needs a preceding image_in()")
        dev = buf["dev_in" + ("16" if buf["bits"] == 16 else "")]
        return dev[8 * self.B:16 * self.B].view(torch.int32).view(self.B, 2)

    def estimate_noise(self, kind: str, into_noise_param: bool = False) -> torch.Tensor:
        """A blind noise-level estimate of every image of the last image_in() batch (SSDN_OP_NOISE_EST, csrc/noise_est.hip) from the
        bytes and tables still on the device.  kind: "gauss" or "poisson" -- what the fp32 parameter in the head's units is (sigma / 255
        or lambda).  into_noise_param: write that parameter into `self.noise_param`, where the head of the next run reads it, without a
        host round trip.  -> the device fp64 tensor [B, 20] (sigma, lambda, n, classes kept, sigma_g[8], m_g[8]; ssdn.utils.estimate_noise
        is the definition), overwritten by the next call; the fp32 parameters [B] are in `self.noise_param` or, without into_noise_param, in
        `self._img["est_param"]`.  Does not synchronise."""
        buf = self._img
        if "offs" not in buf:
            raise L.SsdnHipError("estimate_noise: needs a preceding image_in()")
        if buf["bits"] == 16:
            raise L.SsdnHipError("estimate_noise: " + L.NOISE_EST_BYTES_ONLY)
        if kind not in L.NOISE_EST_KIND:
            raise L.SsdnHipError("estimate_noise: kind must be gauss or poisson, got %r" % (kind,))
        B = self.B
        if "est" not in buf:
            buf["est_hist"] = torch.zeros((B, L.NOISE_EST_CLASSES, L.NOISE_EST_BINS), dtype=torch.int32, device=self.device)
            buf["est_ssum"] = torch.zeros((B, L.NOISE_EST_CLASSES), dtype=torch.int64, device=self.device)
            buf["est"] = torch.zeros((B, L.NOISE_EST_NEST), dtype=torch.float64, device=self.device)
            buf["est_param"] = torch.zeros((B,), dtype=torch.float32, device=self.device)
        dev = buf["dev_in"]
        par = self.noise_param if into_noise_param else buf["est_param"]
        arg = L.NoiseEstArgs(_ptr(dev, buf["head"]), buf["bytes"], _ptr(dev), _ptr(dev, 8 * B), B, self.C, self.H, self.W,
                             L.NOISE_EST_KIND[kind], _ptr(buf["est_hist"]), _ptr(buf["est_ssum"]), _ptr(buf["est"]), _ptr(par))
        OpList([("noise_est", arg)]).run(current_stream())       # (behind image_in()'s upload, on torch's current stream)
        return buf["est"]

    def _head_addend(self, on: bool) -> None:
        """input_grad engines: whether the first network input gradient of the sum adds the head term the VJP left in `dx`"""
        if not self.input_grad or self.pipeline != "ssdn":
            return
        first = self.sigma if self.sigma is not None else self.main
        first.input_grad_args.add = _ptr(self.dx) if on else None

    def backward(self, stream=None, exchange=None, defer_tail=False, with_head_dx=False):
        """Enqueue the backward pass.  exchange (ssdn.hip.dp.GradExchange, overlapped): the main net's list then carries one
        event record per gradient bucket; the last bucket (sigma estimator / learnable sigma) is marked after its own list.
        defer_tail (single-GPU training step only): the last bucket's slab reductions are left to the NEXT adam() call, which runs
        them in front of the optimiser launch -- the flat gradient is incomplete until then.
        with_head_dx (vjp_backward(want_dx=True)): the input gradient adds the head term the VJP has just written into `dx`."""
        s = current_stream() if stream is None else stream
        self._head_addend(with_head_dx)
        if self.accumulate and self.stages_est:     # grads[est_off] += this pass's g_est (the forward's, or the VJP's that replaced it)
            self._accum_ops.run(s)
        if defer_tail and exchange is None and self.ops_opt_tail is not None:
            if self.sigma is not None and (int(self.SIGMA_CONCURRENT) & 2):
                ev = self._fork_sigma(s, self.sigma.bwd)
                self.main.bwd_head.run(s)
                self._join_sigma(s, ev)
            else:
                self.main.bwd_head.run(s)
                if self.sigma is not None:
                    self.sigma.bwd.run(s)
            self._held_input_grad(s)
            self._tail_pending = True
            return
        self._tail_pending = False
        if exchange is not None and exchange.overlapped:
            NB = N_MAIN_BUCKETS
            if getattr(self, "_bwd_ev_key", None) != id(exchange):
                exchange.reset_marks()
                self._bwd_ev = self.main.bwd_with_events(bucket_layers(self.main.plan.layers), exchange.new_event)
                self._bwd_ev_key = id(exchange)
                if len(exchange.ranges) > NB:
                    exchange.record_here(NB)           # (creates the sigma bucket's mark; re-recorded behind its backward list below)
                # the marks belong to THIS engine's list (an exchange may serve several engines, one per input shape)
                self._bwd_ev_marks = (exchange.events, exchange.waits, exchange._here)
                self._bwd_ev_groups = [list(g) for g in self._bwd_ev.coincident] + [[k] for k in range(NB, len(exchange.ranges))]
            exchange.events, exchange.waits, exchange._here = self._bwd_ev_marks
            exchange.groups = self._bwd_ev_groups
            self._bwd_ev.run(s)
            if self.sigma is not None:
                self.sigma.bwd.run(s)
            if len(exchange.ranges) > NB:
                exchange.record_here(NB)
            self._held_input_grad(s)
            return
        if self.sigma is not None and (int(self.SIGMA_CONCURRENT) & 2):
            ev = self._fork_sigma(s, self.sigma.bwd)
            self.main.bwd.run(s)
            self._join_sigma(s, ev)
        else:
            self.main.bwd.run(s)
            if self.sigma is not None:
                self.sigma.bwd.run(s)
        self._held_input_grad(s)

    def _held_input_grad(self, s: int) -> None:
        """mode var with input_grad: the main network's SSDN_OP_INPUT_GRAD, behind both backward lists (it adds the sigma network's)"""
        if self.main.input_grad_ops is not None:
            self.main.input_grad_ops.run(s)

    # ---- autograd: any upstream gradient of the pipeline outputs (SSDN_OP_HEAD_VJP / SSDN_OP_MSE_VJP) -------------------------------
    def _vjp_setup(self):
        """the upstream-gradient buffers and the one-op VJP list (built when first needed: eval engines and train_step never pay)"""
        f32 = dict(dtype=torch.float32, device=self.device)
        B, Cn, H, W = self.B, self.C, self.H, self.W
        self.vjp_w = torch.zeros((B,), **f32)
        self.vjp_g_pme = torch.zeros((B, Cn, H, W), **f32)
        self.vjp_g_mu = torch.zeros((B, Cn, H, W), **f32) if self.pipeline == "ssdn" else None
        g32 = _ptr(self.main.tensor("g32"))
        if self.pipeline == "ssdn":
            a = L.HeadVjpArgs()
            a.net_out, a.noisy, a.noise_param = _ptr(self.main.tensor("out32")), _ptr(self.inp), _ptr(self.noise_param)
            a.B, a.C, a.H, a.W, a.style, a.mode = B, Cn, H, W, STYLE[self.style], MODE[self.mode]
            a.nchunks, a.g_net_out, a.partial, a.gmax = self.nchunks, g32, _ptr(self.partial), self._gmax(self.main)
            a.diag = int(self.diag)
            if self.mode == "const":
                a.est_raw, a.g_est = _ptr(self.params, 4 * self.est_off), self._g_est_ptr()
            elif self.mode == "var":
                a.est_raw, a.g_est = _ptr(self.est_raw), _ptr(self.g_est_var)
                a.g_sigma_out, a.gmax2 = _ptr(self.sigma.tensor("g32")), self._gmax(self.sigma)
            self._vjp = (a, OpList([("head_vjp", a)]))
        else:
            a = L.MseVjpArgs(_ptr(self.main.tensor("out32")), _ptr(self.ref), _ptr(self.coords), self.ncoords, int(self.pipeline == "mask_mse"),
                             B, Cn, H, W, 0, None, None, g32, self._gmax(self.main))
            self._vjp = (a, OpList([("mse_vjp", a)]))

    def vjp_backward(self, w: Optional[torch.Tensor] = None, g_pme: Optional[torch.Tensor] = None, g_mu: Optional[torch.Tensor] = None,
                     stream=None, want_dx: bool = False):
        """Backward pass for ANY upstream gradient of the last training forward: w = dL/dLOSS [B] (or [B,1]), g_pme = dL/dIMG_DENOISED,
        g_mu = dL/dIMG_MU (ssdn), [B,C,H,W]; None = no gradient for that output.  Enqueues the VJP op (the loss gradient g32, the
        sigma partials and g_est), then the backward lists.  w == 1/B alone (mean(LOSS)) leaves the forward's loss gradient in place
        (decided on the device): then the result is bit-identical to backward().
        want_dx (engines built with input_grad=True): the pass also leaves dL/d(noisy input) in `self.dx` (the head's direct term via
        the VJP's g_noisy, then the networks' input gradients).  The parameter gradients are the same, bit for bit, either way."""
        if not self.train:
            raise L.SsdnHipError("vjp_backward needs a training engine")
        if want_dx and not self.input_grad:
            raise L.SsdnHipError("vjp_backward(want_dx=True) needs an engine built with input_grad=True")
        if self._vjp is None:
            self._vjp_setup()
        a, ops = self._vjp
        a.w = a.g_pme = None
        if w is not None:
            self.vjp_w.copy_(w.reshape(self.B), non_blocking=True)
            a.w = _ptr(self.vjp_w)
        if g_pme is not None:
            self.vjp_g_pme.copy_(g_pme, non_blocking=True)
            a.g_pme = _ptr(self.vjp_g_pme)
        if self.pipeline == "ssdn":
            a.g_mu = None
            if g_mu is not None:
                self.vjp_g_mu.copy_(g_mu, non_blocking=True)
                a.g_mu = _ptr(self.vjp_g_mu)
            a.g_noisy = _ptr(self.dx) if want_dx else None
        elif g_mu is not None:
            raise L.SsdnHipError("the %s pipeline has no IMG_MU" % self.pipeline)
        a.keep = int(self.g_fresh)
        s = current_stream() if stream is None else stream
        ops.run(s)
        self.g_fresh = False
        self.backward(stream=s, with_head_dx=want_dx and self.pipeline == "ssdn")

    def adam(self, lr: float, step: int, gscale: float = 1.0, stream=None):
        for a in self._adam_args:
            a.lr, a.bc1, a.bc2, a.gscale = lr, 1.0 - 0.9 ** step, 1.0 - 0.99 ** step, gscale
        s = current_stream() if stream is None else stream
        if self._tail_pending:                # (the deferred reductions of the last bucket, then the optimiser launch)
            self._tail_pending = False
            self.ops_opt_tail.run(s)
            return
        self.ops_opt.run(s)                   # optimiser step + re-pack of the MFMA shadows (one launch per network)
