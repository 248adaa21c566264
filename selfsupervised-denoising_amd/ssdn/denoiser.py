"""`Denoiser` -- network(s) + loss head of one ssdn configuration, MI355X edition.

Drop-in for /root/reference/ssdn/ssdn/denoiser.py:23-412: same constructor (`cfg`, `device`), `run_pipeline`, `forward`,
`get_model`, `state_dict` / `from_state_dict` (same key layout incl. the DataParallel `module.` prefix and the `_models`
aliases) and `config_name`.  What differs is everything underneath: the nets' parameters are views
into ONE flat fp32 device buffer [main net | sigma estimator | learnable sigma scalar]; a forward / loss / backward /
optimiser step is four calls into libssdn_hip.so (`ssdn.hip.engine.DenoiserEngine`); nn.DataParallel is gone -- data
parallelism is one process per GPU with an RCCL all-reduce of the flat gradient (`ssdn.hip.dp`).

Autograd: a training-mode `run_pipeline` / `forward` with grad enabled returns LOSS, IMG_DENOISED and IMG_MU (MSE pipelines: LOSS when
there is a reference, and IMG_DENOISED) as outputs of one autograd node.  So does a run in ANY mode (eval() included) with grad enabled
whose noisy input `data[0]` requires grad: the input is then an input of that node too, and its backward returns dL/d(input) -- the
loss head's direct dependence on the noisy image plus the input gradients of the main network and, for a variable noise level, of the
sigma estimator, summed on the device in one fixed order -- in the input's dtype and on its device, where torch
accumulates it into `.grad`.  Such a run uses a training plan with input gradients for that shape; in eval() it does not become the
forward that `Denoiser.backward()` / `optimizer_step()` act on, and its outputs equal those of the same eval-mode run under no_grad.  Its backward takes ANY upstream gradient of them -- per-sample
weights or other reductions of LOSS, a loss on the posterior mean or on mu, or several at once -- copies those that arrived into the
engine and runs the vector-Jacobian product of the loss head on the GPU (SSDN_OP_HEAD_VJP / SSDN_OP_MSE_VJP), then the planned
backward pass.  `torch.mean(LOSS).backward()` gives exactly the gradient of `Denoiser.backward()`.  The parameters' `.grad` are views
of the flat gradient buffer.

Gradient accumulation.  With `accumulate_grads = False` (the default) every backward OVERWRITES the flat gradient, so all terms of a
loss go through ONE `backward()` call -- eval-mode input-gradient graphs too.  With `accumulate_grads = True`, `Denoiser.backward()`
and the autograd node ADD into it until `zero_grad()` / `optimizer_step()`: torch's `.grad` semantics, so several losses may go through
several backward calls (as forward, backward, forward, backward: a pass decides whether it adds when its FORWARD is enqueued, and in
mode const a backward that must add although its forward has already overwritten the scalar's gradient raises).  The first pass into a clean buffer overwrites (there is no zero-fill
launch and stale values never leak in); after passes 1..K the buffer holds fl(..fl(fl(g_1 + g_2) + g_3).. + g_K) element by
element, g_k being bit for bit what pass k alone writes (the slab reductions add in their epilogue, ssdn_wreduce_args.accumulate; the
learnable noise scalar goes through a staging float and SSDN_OP_ACCUM).  A `torch.optim` optimiser's
`zero_grad(set_to_none=True)` drops the `.grad` handles without telling the module: a pass that finds them gone treats the buffer as
clean.  `accumulate_step` adds one micro-batch (forward + loss + backward, no exchange, no optimiser step, no re-pack) whatever
`accumulate_grads` says; the `train_step` that follows adds its own, exchanges once and steps Adam once on the MEAN over the
micro-batches (gscale = 1 / ((n + 1) * world)).  The input gradient is per forward and never accumulated here (torch's AccumulateGrad
does that for the caller).  A graph whose engine has since run another training forward (`run_pipeline`
or `train_step` of the same shape, or another input-gradient run of that shape) raises RuntimeError on backward.  The planned route `Denoiser.backward()` consumes its forward: afterwards that forward's IMG_DENOISED
and IMG_MU are plain tensors again (detached in place), as they always were on that route.  NOISE_STD_DEV and MODEL_STD_DEV, no_grad outputs, eval-mode outputs of an input that does not require
grad and everything `train_step` returns carry no graph (train_step never computes an input gradient).  No gradient flows into the
reference image, the noise metadata or the std-dev outputs.
"""
from __future__ import annotations

import math
import weakref
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn
from torch import Tensor
from torch.autograd.function import once_differentiable

import ssdn
from ssdn.datasets import NoisyDataset
from ssdn.hip.lib import NOISE_EST_BYTES_ONLY
from ssdn.models import NoiseNetwork
from ssdn.params import ConfigValue, NoiseValue, Pipeline, PipelineOutput

_MAX_ENGINES = 4        # cached (batch, size, mode) plans per Denoiser; the least recently used one is dropped beyond this


class _ParallelShim(nn.Module):
    """Occupies the place of nn.DataParallel in the module tree so that checkpoints keep the
    `models.<id>.module.<param>` key layout (denoiser.py:102-110).  It parallelises nothing."""

    def __init__(self, module: nn.Module):
        super().__init__()
        self.module = module

    def forward(self, *a, **k):
        return self.module(*a, **k)


class _PipelineGrad(torch.autograd.Function):
    """The differentiable outputs of one training-mode pipeline run (`names`: LOSS / IMG_DENOISED / IMG_MU) as one node.  Its backward
    hands whichever upstream gradients arrived (None = that output was not used) to the engine that PRODUCED them, which runs the
    head's vector-Jacobian product and the planned backward lists; the parameters' `.grad` then show the flat gradient buffer."""

    @staticmethod
    def forward(ctx, anchor: Tensor, x: Optional[Tensor], denoiser: "Denoiser", engine, names: Tuple, *outs: Tensor):
        # x: the caller's noisy input when it requires grad (the engine then has input gradients), else None
        ctx.set_materialize_grads(False)
        ctx.denoiser, ctx.engine, ctx.names, ctx.gen = denoiser, engine, names, engine.gen
        ctx.x_dtype, ctx.x_device = (x.dtype, x.device) if x is not None else (None, None)
        return tuple(o.clone() for o in outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        eng = ctx.engine
        if eng.gen != ctx.gen:
            raise RuntimeError("Denoiser: the buffers of this graph were overwritten by a later training forward (run_pipeline or "
                               "train_step) of the same input shape; run backward before the next training forward of that shape")
        g = dict(zip(ctx.names, grads))
        want_dx = bool(ctx.needs_input_grad[1])
        ctx.denoiser._backward_engine(eng, g.get(PipelineOutput.LOSS), g.get(PipelineOutput.IMG_DENOISED), g.get(PipelineOutput.IMG_MU),
                                      want_dx=want_dx)
        dx = eng.dx.clone().to(device=ctx.x_device, dtype=ctx.x_dtype) if want_dx else None   # (the next backward overwrites eng.dx)
        return (None, dx, None, None, None) + (None,) * len(grads)


class Denoiser(nn.Module):
    MODEL = "denoiser_model"
    SIGMA_ESTIMATOR = "sigma_estimation_model"
    ESTIMATED_SIGMA = "estimated_sigma"

    def __init__(self, cfg: Dict, device: str = None):
        super().__init__()
        self.device = torch.device(device) if device else torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.cfg = cfg
        C = cfg[ConfigValue.IMAGE_CHANNELS]
        self._pipeline = cfg[ConfigValue.PIPELINE]
        ssdn_pipe = self._pipeline == Pipeline.SSDN
        # DIAGONAL_COVARIANCE: means + the diagonal of A (denoiser.py:57-58; the loss head of DESIGN.md section 3.10 -- the reference's own
        # diagonal branch raises at `c00.shape()`, denoiser.py:240).  The MSE pipelines ignore it, as the reference does.
        self._diag = bool(ssdn_pipe and cfg.get(ConfigValue.DIAGONAL_COVARIANCE))
        if self._diag and str(cfg.get(ConfigValue.NOISE_STYLE) or "").startswith("impulse"):
            raise NotImplementedError("DIAGONAL_COVARIANCE is not implemented for the impulse noise model (the head refuses diag = 1 with "
                                      "style = 2)")
        if self._diag:
            cout = 2 * C
        else:
            cout = C + (C * (C + 1)) // 2 if ssdn_pipe else C           # means + triangular A (denoiser.py:55-64)
        self._var = ssdn_pipe and cfg[ConfigValue.NOISE_VALUE] == NoiseValue.UNKNOWN_VARIABLE
        self._const = ssdn_pipe and cfg[ConfigValue.NOISE_VALUE] == NoiseValue.UNKNOWN_CONSTANT
        blind = cfg[ConfigValue.BLINDSPOT]
        from ssdn.hip.graph import net_layers, net_param_count
        n_main = net_param_count(net_layers(C, cout, blind))
        n_sig = net_param_count(net_layers(C, 1, False)) if self._var else 0
        n_tot = n_main + n_sig + (1 if self._const else 0)
        n_pad = (n_tot + 3) // 4 * 4
        self._n_main, self._n_sig = n_main, n_sig
        self.flat = torch.zeros(n_pad, device=self.device)
        self.flat_grad = torch.zeros(n_pad, device=self.device)
        self.adam_m = torch.zeros(n_pad, device=self.device)
        self.adam_v = torch.zeros(n_pad, device=self.device)
        self.adam_steps = 0

        self.models = nn.ModuleDict()    # "parallelised" handles (reference: nn.DataParallel wrappers)
        self._models = nn.ModuleDict()   # plain handles to the same modules
        self._add(Denoiser.MODEL, NoiseNetwork(C, cout, blindspot=blind, device=self.device,
                                               flat=(self.flat[:n_main], self.flat_grad[:n_main])))
        if self._var:
            self._add(Denoiser.SIGMA_ESTIMATOR, NoiseNetwork(C, 1, blindspot=False, zero_output_weights=True, device=self.device,
                                                            flat=(self.flat[n_main:n_main + n_sig], self.flat_grad[n_main:n_main + n_sig])))
        self.l_params = nn.ParameterDict()
        if self._const:
            self.l_params[Denoiser.ESTIMATED_SIGMA] = nn.Parameter(self.flat[n_main + n_sig:n_main + n_sig + 1].view(1, 1, 1, 1))
        self._engines: Dict[Tuple, list] = {}       # key -> [engine, parameter version its 16-bit weight shadows hold]
        self._version = 0
        self._last_engine = None                     # engine of the last run_pipeline (any mode)
        self._last_train_engine = None               # engine of the last TRAINING-mode run_pipeline (backward / optimiser)
        self._exchange = None                        # ssdn.hip.dp.GradExchange of train_step (data parallel)
        self._anchor = torch.zeros((), requires_grad=True)
        self._img_graph = None                       # (engine, generation, weak refs to IMG_DENOISED / IMG_MU) of the last autograd forward
        # gradient accumulation: backward() and the autograd node add into flat_grad (torch's .grad semantics) instead of overwriting it
        self.accumulate_grads = False
        self._grad_terms = 0                         # backward results currently summed in flat_grad (0 = clean: the next pass overwrites)
        self._grads_exposed = False                  # the parameters' .grad handles show flat_grad (_expose_grads)

    def _add(self, model_id: str, model: nn.Module):
        self._models[model_id] = model
        self.models[model_id] = _ParallelShim(model)

    # ---- reference surface --------------------------------------------------------------------------------------
    def get_model(self, model_id: str, parallelised: bool = True) -> nn.Module:
        return (self.models if parallelised else self._models)[model_id]

    def config_name(self) -> str:
        return ssdn.cfg.config_name(self.cfg)

    def state_dict(self, params_only: bool = False, **kw) -> Dict:
        sd = super().state_dict(**kw)
        if not params_only:
            sd["cfg"] = self.cfg
        return sd

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        sd = {k: v for k, v in state_dict.items() if k != "cfg"}
        r = super().load_state_dict(sd, strict=strict, **kw)
        self.mark_dirty()
        return r

    @staticmethod
    def from_state_dict(state_dict: Dict) -> "Denoiser":
        d = Denoiser(state_dict["cfg"])
        d.load_state_dict(state_dict, strict=False)
        return d

    def mark_dirty(self):
        """The fp32 parameters changed: the fp16/bf16 MFMA shadows are re-packed before the next run.  In-place updates of the
        parameters themselves (a `torch.optim` step, `load_state_dict`, `p.copy_()` under no_grad) are detected through the version
        counter of the flat buffer, which all parameter views share.  Writes through `p.data` (its own version counter) or a raw
        pointer are NOT: call this after them.  Evaluation-mode runs re-pack unconditionally (23 us), so a stale shadow can only
        ever be seen by a training-mode forward that follows an undeclared `.data` write."""
        self._version += 1
        for m in self._models.values():
            if hasattr(m, "mark_dirty"):
                m.mark_dirty()

    # ---- gradient accumulation -------------------------------------------------------------------------------------
    def zero_grad(self, set_to_none: bool = True):
        """Marks the flat gradient clean: the next backward overwrites it (nothing is zero-filled for that), then nn.Module.zero_grad."""
        self._grad_terms = 0
        self._grads_exposed = False
        n_tot = self._n_main + self._n_sig + (1 if self._const else 0)
        if n_tot < self.flat_grad.numel():       # (the <= 3 padding floats behind the last parameter have no writer in any pass)
            self.flat_grad[n_tot:].zero_()
        return super().zero_grad(set_to_none=set_to_none)

    def _adds(self, force: bool = False) -> bool:
        """whether a pass enqueued now adds to flat_grad: accumulation is wanted (accumulate_grads, or force: accumulate_step / the
        train_step behind it) and the buffer holds a sum.  A torch.optim zero_grad(set_to_none=True) has dropped the exposed `.grad`
        handles (all at once: one check is enough) while the buffer kept the old sum: that counts as clean."""
        if not (force or self.accumulate_grads) or self._grad_terms == 0:
            return False
        if self._grads_exposed:
            net = self._models[Denoiser.MODEL]
            if net.get_submodule(net.layers[0].name).weight.grad is None:
                self._grad_terms, self._grads_exposed = 0, False
                return False
        return True

    def _sync_accumulate(self, eng, adds: bool) -> bool:
        """A backward whose forward was enqueued under the other decision (another shape's backward, or a zero_grad, came in between).
        The slab reductions take the flag at any time.  Mode const: a forward that staged g_est can still overwrite (-> True: the caller
        goes through the VJP, which rewrites g_est where it now points); one that stored it into the running sum cannot be undone."""
        if eng.accumulate == adds:
            return False
        if eng.stages_est and adds:
            raise RuntimeError("Denoiser: with a learnable noise scalar the forward of an accumulating backward must be enqueued after the "
                               "backward before it (forward, backward, forward, backward): this forward overwrote the scalar's gradient")
        eng.set_accumulate(adds)
        return eng.stages_est

    def _count_backward(self, adds: bool) -> None:
        if self.accumulate_grads:
            self._grad_terms = self._grad_terms + 1 if adds else 1
        else:
            self._grad_terms = 0

    def _param_version(self):
        return (self._version, self.flat._version)

    # ---- engines ---------------------------------------------------------------------------------------------------
    def _engine(self, B: int, H: int, W: int, train: bool, ncoords: int = 64, input_grad: bool = False, repack: bool = False):
        from ssdn.hip import lib as L
        from ssdn.hip.engine import DenoiserEngine
        if self.device.type != "cuda":
            raise L.SsdnHipError("Denoiser.run_pipeline needs an MI355X: device is %s and the ssdn hot path has no CPU fallback" % self.device)
        key = (B, H, W, train, ncoords) + ((True,) if input_grad else ())        # (input-gradient plans: a key of their own)
        if key not in self._engines:
            cfg = self.cfg
            eng = DenoiserEngine(self._pipeline.value, cfg[ConfigValue.IMAGE_CHANNELS], cfg[ConfigValue.BLINDSPOT],
                                 cfg.get(ConfigValue.NOISE_STYLE) or "gauss", cfg[ConfigValue.NOISE_VALUE].value if self._pipeline == Pipeline.SSDN else "known",
                                 B, H, W, self.device, self.flat, self.flat_grad, self.adam_m, self.adam_v,
                                 self._n_main, self._n_sig, self._const, train=train, ncoords=ncoords, input_grad=input_grad,
                                 diag=self._diag)
            self._engines[key] = [eng, None]
            while len(self._engines) > _MAX_ENGINES:         # LRU: a plan owns ~1 GB of buffers at BASELINE sizes
                old = next(k for k in self._engines if k != key)
                dead = self._engines.pop(old)[0]
                if dead is self._last_engine:
                    self._last_engine = None
                if dead is self._last_train_engine:
                    self._last_train_engine = None
        slot = self._engines.pop(key)
        self._engines[key] = slot                            # most recently used last
        if slot[1] != self._param_version() or not train or repack:
            slot[0].repack()
            slot[1] = self._param_version()
        return slot[0]

    # ---- pipelines -------------------------------------------------------------------------------------------------
    def forward(self, data: Tensor) -> Tensor:
        """Inference (denoiser.py:112-126): denoise a BCHW batch with the configured pipeline."""
        return self.run_pipeline([data])[PipelineOutput.IMG_DENOISED]

    def run_pipeline(self, data: List, **kwargs) -> Dict:
        """Reference surface (denoiser.py:128-138).  Outputs are fresh tensors, as in the reference: the caller may keep
        them across calls.  (`train_step` uses the engine's buffers directly.)"""
        return self._run(data, clone=True)

    def input_buffer(self, B: int, H: int, W: int, ncoords: int = 64) -> Optional[Tensor]:
        """The fp32 [B, C, H, W] input buffer of the TRAINING engine for this shape.  A producer that writes the noisy minibatch
        straight into it (ssdn.datasets.DevicePatchStream does, when attached) and passes that very tensor as the pipeline
        input saves `run_pipeline` its device-to-device copy; the buffer is overwritten by the next minibatch.
        Never BUILDS an engine (a plan owns ~1 GB) and never touches the LRU order or the weight shadows: None until the first
        training step of this shape has created it (the producer then uses a buffer of its own, once)."""
        slot = self._engines.get((B, H, W, True, ncoords))
        return slot[0].inp if slot is not None else None

    def _run(self, data: List, clone: bool, bridge: bool = True, accumulate: bool = False) -> Dict:
        if self._pipeline not in (Pipeline.MSE, Pipeline.SSDN, Pipeline.MASK_MSE):
            raise NotImplementedError("Unsupported processing pipeline")
        inp = data[NoisyDataset.INPUT]
        B, C, H, W = inp.shape
        ref = data[NoisyDataset.REFERENCE] if len(data) > NoisyDataset.REFERENCE else None
        meta = data[NoisyDataset.METADATA] if len(data) > NoisyDataset.METADATA else {}
        MD = NoisyDataset.Metadata
        coords = meta.get(MD.MASK_COORDS) if isinstance(meta, dict) else None
        if coords is not None and coords.device.type == "cpu" and coords.numel():
            c0 = coords[0]          # the reference indexes with batch element 0's coordinates and raises IndexError out of range
            if int(c0[:, 0].min()) < -H or int(c0[:, 0].max()) >= H or int(c0[:, 1].min()) < -W or int(c0[:, 1].max()) >= W:
                raise IndexError("mask coordinates out of range for a %dx%d image" % (H, W))
        train = self.training and torch.is_grad_enabled()
        # an input that requires grad (any mode; never train_step): a training plan with input gradients, x an input of the graph.  In
        # eval() the shadows are re-packed as for every eval-mode run, and the run does not become the last training forward
        want_x = bridge and torch.is_grad_enabled() and inp.requires_grad
        eng = self._engine(B, H, W, train or want_x, ncoords=(coords.shape[1] if coords is not None else 64), input_grad=want_x,
                           repack=want_x and not train)
        if inp.data_ptr() != eng.inp.data_ptr():                          # (a producer may have written the engine's buffer itself)
            # detached: the engine's persistent buffer (input_buffer(), the sigma network's input) never joins the caller's graph
            eng.inp.copy_(inp.detach().to(torch.float32), non_blocking=True)      # device boundary (denoiser.py:143,186)
        have_loss = True
        if self._pipeline == Pipeline.SSDN:
            if self.cfg[ConfigValue.NOISE_VALUE] == NoiseValue.KNOWN:
                npv = meta[MD.INPUT_NOISE_VALUES]
                # A producer may mark a parameter tensor it never rewrites (DevicePatchStream's cached constant of a fixed-sigma style:
                # `_ssdn_const`); that very OBJECT (held by reference, so its address cannot be handed out again) is uploaded once.
                # Everything else -- e.g. the per-minibatch tensor of a ranged style, filled through a raw pointer, whose
                # (address, _version) can repeat with different contents -- is copied every step (B floats, device to device).
                if npv.data_ptr() == eng.noise_param.data_ptr():       # (denoise's "auto": the estimator has written the engine's tensor itself)
                    eng._np_src = None
                elif not (getattr(npv, "_ssdn_const", False) and npv is getattr(eng, "_np_src", None)):
                    if getattr(npv, "_ssdn_per_sample", False):        # (DevicePoolStream's per-image table: [B,C,1,1], one value per sample in every channel)
                        npv = npv.reshape(B, -1)[:, 0]
                    eng.noise_param.copy_(npv.reshape(B).to(torch.float32), non_blocking=True)
                    eng._np_src = npv if getattr(npv, "_ssdn_const", False) else None
        else:
            have_loss = ref is not None and (self._pipeline == Pipeline.MSE or coords is not None)
            if have_loss:
                eng.ref.copy_(ref.to(torch.float32), non_blocking=True)
                if self._pipeline == Pipeline.MASK_MSE:
                    c0 = coords[0].to(torch.int64)
                    c0 = torch.stack([c0[:, 0] % H, c0[:, 1] % W], 1)              # python-style negative indices wrap
                    eng.coords.copy_(c0, non_blocking=True)   # element 0's mask for everyone (n2v_loss.py:12)
        if eng.train:                      # (whether this pass adds is decided here: in mode const the forward's loss op stores g_est)
            eng.set_accumulate(self._adds(force=accumulate))
        if have_loss:
            eng.forward()
        else:
            eng.net_forward_only()
        self._last_engine = eng
        self._has_loss_last = have_loss
        if train:
            self._last_train_engine = eng
        own = (lambda t: t.clone()) if clone else (lambda t: t)
        diff = {}
        if (train and bridge) or want_x:
            # the differentiable outputs, through one autograd node (which clones them); train_step (bridge=False) has no graph
            names = ((PipelineOutput.LOSS,) if have_loss else ()) + ((PipelineOutput.IMG_DENOISED, PipelineOutput.IMG_MU)
                                                                     if self._pipeline == Pipeline.SSDN else (PipelineOutput.IMG_DENOISED,))
            src = {PipelineOutput.LOSS: eng.loss, PipelineOutput.IMG_MU: eng.mu,
                   PipelineOutput.IMG_DENOISED: eng.pme if self._pipeline == Pipeline.SSDN else eng.main.tensor("out32")}
            diff = dict(zip(names, _PipelineGrad.apply(self._anchor, inp if want_x else None, self, eng, names, *[src[n] for n in names])))
            if train:                    # (what Denoiser.backward() consumes: the last TRAINING forward's images)
                self._img_graph = (eng, eng.gen, [weakref.ref(diff[n]) for n in names if n != PipelineOutput.LOSS])
        pick = lambda n, t: diff[n] if n in diff else own(t)   # noqa: E731
        out = {PipelineOutput.INPUTS: data}
        net_out = eng.main.tensor("out32")
        if self._pipeline == Pipeline.SSDN:
            out[PipelineOutput.IMG_MU] = pick(PipelineOutput.IMG_MU, eng.mu)
            out[PipelineOutput.IMG_DENOISED] = pick(PipelineOutput.IMG_DENOISED, eng.pme)
            nstd = eng.noise_std
            if eng.style != "poisson":                   # gauss: sigma, impulse: alpha -- one value per sample
                nstd = nstd[:1].view(1, 1, 1) if self._const else nstd.view(B, 1, 1)
            out[PipelineOutput.NOISE_STD_DEV] = own(nstd)
            out[PipelineOutput.MODEL_STD_DEV] = own(eng.model_std)
        else:
            out[PipelineOutput.IMG_DENOISED] = pick(PipelineOutput.IMG_DENOISED, net_out)
        if have_loss:
            # (train_step drives the backward list itself: no autograd node, no copy of the loss)
            out[PipelineOutput.LOSS] = pick(PipelineOutput.LOSS, eng.loss)
        return out

    def posterior(self, data, samples: int = 0, seed: int = 0, offset: int = 0) -> Dict:
        """The per-pixel posterior of the SSDN head for a BCHW batch (or a pipeline `data` list): N(mean, cov) per pixel, for the impulse
        model the two-component mixture's mean and covariance.  -> {"mean": IMG_DENOISED [B,C,H,W], "cov": [B, C(C+1)/2, H, W] (upper
        triangle: 00, 01, 02, 11, 12, 22), "std": [B,C,H,W]} and, for samples > 0, "samples": [samples, B, C, H, W] posterior draws -- a
        pure function of (seed, offset, sample index, pixel), so pass a fresh offset for fresh draws.  Runs an inference plan under
        no_grad whatever the module's mode: it never becomes the forward that backward() / optimizer_step() / accumulate_metrics() act
        on.  Plain, fresh tensors; nothing is differentiable.  SSDN pipeline only."""
        if self._pipeline != Pipeline.SSDN:
            raise NotImplementedError("Denoiser.posterior: the %s pipeline has no posterior covariance (SSDN pipeline only)" % self._pipeline.value)
        samples = int(samples)
        if samples < 0:
            raise ValueError("samples must be >= 0")
        if isinstance(data, Tensor):
            data = [data]
        keep = (self._last_engine, getattr(self, "_has_loss_last", None))
        try:
            with torch.no_grad():
                out = self._run(data, clone=True)           # (no_grad: an inference plan; _last_train_engine is left alone)
                res = {k: v.clone() for k, v in self._last_engine.posterior(n_samples=samples, seed=seed, offset=offset).items()}
        finally:
            self._last_engine, self._has_loss_last = keep
        res["mean"] = out[PipelineOutput.IMG_DENOISED]
        return res

    def _noise_param_value(self, noise_param) -> Optional[float]:
        """`denoise`'s noise_param as the value Metadata.INPUT_NOISE_VALUES carries: the numeric part of the model's noise style in
        the style grammar (ssdn.utils.noise.parse_style) -- gauss: an integer is /255; poisson: lambda; impulse: an integer is per
        cent.  Required for a known-noise SSDN model and refused for every other one (ValueError).  "auto" (gauss and poisson models
        only: there is no estimator for impulse noise) comes back as it is: `denoise` then estimates the value per image on the device."""
        from ssdn.utils import noise
        known = self._pipeline == Pipeline.SSDN and self.cfg[ConfigValue.NOISE_VALUE] == NoiseValue.KNOWN
        if not known:
            if noise_param is not None:
                raise ValueError("denoise: noise_param is for ssdn models trained with a known noise parameter; this model takes none")
            return None
        if noise_param is None:
            raise ValueError("denoise: this model was trained with a known noise parameter: noise_param is required")
        kind = noise.parse_style(self.cfg[ConfigValue.NOISE_STYLE])[0]
        if isinstance(noise_param, str) and noise_param.strip().lower() == "auto":
            if kind not in ("gauss", "poisson"):
                raise ValueError("denoise: noise_param 'auto' needs a noise-level estimator and no estimator exists for %s noise: "
                                 "pass the number" % kind)
            return "auto"
        try:
            params = noise.parse_style(kind + str(noise_param).strip())[1]
        except (ValueError, IndexError):
            params = []
        if len(params) != 1:
            raise ValueError("denoise: noise_param %r is not one number in the grammar of a %s style" % (noise_param, kind))
        v = params[0]
        if v < 0:
            raise ValueError("denoise: noise_param must not be negative, got %r" % (noise_param,))
        if kind == "gauss":
            return v / 255 if isinstance(v, int) else float(v)
        if kind == "impulse":
            return noise.impulse_alpha(v)
        return float(v)

    def _denoise_images(self, images: List) -> List[Tensor]:
        """`denoise`'s images as contiguous uint8 or uint16 CPU tensors [h, w, C] of the model's channel count (ValueError otherwise)"""
        import numpy as np
        Cn = self.cfg[ConfigValue.IMAGE_CHANNELS]
        imgs = []
        for k, im in enumerate(images):
            t = im
            if isinstance(im, np.ndarray):
                a = np.ascontiguousarray(im)
                t = torch.from_numpy(a if a.flags.writeable else a.copy())      # (PIL hands out read-only arrays)
            if not torch.is_tensor(t) or t.dtype not in (torch.uint8, torch.uint16) or t.dim() not in (2, 3):
                raise ValueError("denoise: image %d is not a uint8 or uint16 array or tensor [h, w] or [h, w, C]" % k)
            t = t.detach().cpu()
            t = (t.unsqueeze(-1) if t.dim() == 2 else t).contiguous()
            if t.shape[2] != Cn:
                raise ValueError("denoise: image %d has %d channel(s), the model takes %d" % (k, t.shape[2], Cn))
            if t.shape[0] < 1 or t.shape[1] < 1:
                raise ValueError("denoise: image %d is empty" % k)
            imgs.append(t)
        return imgs

    @staticmethod
    def _denoise_options(bucket: Optional[int], batch_size: int) -> Tuple[int, int]:
        mul = NoiseNetwork.input_wh_mul()
        bucket = mul if bucket is None else int(bucket)
        if bucket < mul or bucket % mul:
            raise ValueError("denoise: bucket must be a positive multiple of %d, got %d" % (mul, bucket))
        batch_size = int(batch_size)
        if batch_size < 1:
            raise ValueError("denoise: batch_size must be at least 1")
        return bucket, batch_size

    @staticmethod
    def _tile_options(tile: Optional[int], overlap: Optional[int]) -> Tuple[Optional[int], Optional[int]]:
        """`denoise`'s tile and overlap as the (T, O) of SSDN_OP_TILE_IN, or (None, None) without tiling (ValueError otherwise)"""
        mul = NoiseNetwork.input_wh_mul()
        if tile is None:
            if overlap is not None:
                raise ValueError("denoise: overlap needs tile")
            return None, None
        tile = int(tile)
        if tile < mul or tile % mul:
            raise ValueError("denoise: tile must be a positive multiple of %d, got %d" % (mul, tile))
        if overlap is None:
            overlap = min(max(mul, tile // 4 // mul * mul), tile // 2 // mul * mul)
        overlap = int(overlap)
        if overlap < 0 or overlap % mul:
            raise ValueError("denoise: overlap must be a multiple of %d and not negative, got %d" % (mul, overlap))
        if 2 * overlap > tile:
            raise ValueError("denoise: 2 * overlap must not exceed tile, got overlap %d for tile %d" % (overlap, tile))
        return tile, overlap

    def _denoise_groups(self, imgs: List[Tensor], bucket: int, uniform: bool, members: Optional[List[int]] = None) -> Dict[Tuple[int, int], List[int]]:
        """the images' indices (all, or `members`) by padded shape on tensor axes 2 and 3 = along the image's x and y
        (NoisyDataset.get_output_size: uniform, multiple, square)"""
        members = list(range(len(imgs))) if members is None else members
        big = (max(imgs[k].shape[1] for k in members), max(imgs[k].shape[0] for k in members))
        groups: Dict[Tuple[int, int], List[int]] = {}
        for k in members:
            t = imgs[k]
            H, W = ((n + bucket - 1) // bucket * bucket for n in (big if uniform else (t.shape[1], t.shape[0])))
            if self.cfg[ConfigValue.BLINDSPOT]:
                H = W = max(H, W)
            groups.setdefault((H, W), []).append(k)
        return groups

    def estimate_noise(self, images: List, kind: Optional[str] = None, batch_size: int = 1, bucket: Optional[int] = None,
                       uniform: bool = False) -> List[Dict]:
        """A blind estimate of the noise level of every image, on the device (SSDN_OP_NOISE_EST, csrc/noise_est.hip, DESIGN.md section
        3.17; ssdn.utils.estimate_noise is the definition and documents the values).  images, batch_size, bucket, uniform: as for
        `denoise`, whose validation and grouping it shares -- an image only has to fit the engine it is uploaded to.  kind: "gauss" or
        "poisson", default the model's noise style; an impulse model needs it given (ValueError), there is no impulse estimator.
        -> per image {"sigma" (byte units), "lambda", "n", "classes_used", "nlf_sigma" [8], "nlf_mean" [8]} and "noise_param": the
        fp32 value of `kind` in the head's units (sigma / 255 or lambda) as a float, NaN for an image with fewer than 256 valid
        windows.  Runs no network and leaves training state and the last forward alone."""
        from ssdn.utils import noise
        if kind is None:
            kind = noise.parse_style(self.cfg.get(ConfigValue.NOISE_STYLE) or "gauss")[0]
            if kind not in ("gauss", "poisson"):
                raise ValueError("estimate_noise: no estimator exists for %s noise: pass kind='gauss' or 'poisson'" % kind)
        if kind not in ("gauss", "poisson"):
            raise ValueError("estimate_noise: kind must be 'gauss' or 'poisson', got %r" % (kind,))
        bucket, batch_size = self._denoise_options(bucket, batch_size)
        imgs = self._denoise_images(images)
        if any(t.dtype == torch.uint16 for t in imgs):
            raise ValueError("estimate_noise: " + NOISE_EST_BYTES_ONLY)
        res: List = [None] * len(imgs)
        if not imgs:
            return res
        with torch.no_grad():
            for (H, W), members in self._denoise_groups(imgs, bucket, uniform).items():
                for lo in range(0, len(members), batch_size):
                    idx = members[lo:lo + batch_size]
                    eng = self._engine(len(idx), H, W, False)
                    eng.image_in([imgs[k] for k in idx])
                    est = eng.estimate_noise(kind).cpu()             # (synchronises)
                    par = eng._img["est_param"].cpu()
                    for b, k in enumerate(idx):
                        res[k] = self._noise_est_dict(est[b], float(par[b]))
        return res

    @staticmethod
    def _noise_est_dict(row: Tensor, param: float) -> Dict:
        """one row of SSDN_OP_NOISE_EST's `est` (host float64 [20]) as ssdn.utils.estimate_noise's dict, plus the fp32 parameter"""
        return {"sigma": float(row[0]), "lambda": float(row[1]), "n": int(row[2]), "classes_used": int(row[3]),
                "nlf_sigma": row[4:12].clone(), "nlf_mean": row[12:20].clone(), "noise_param": param}

    def _tile_buffer(self, name: str, numel: int, dtype, pinned: bool = False) -> Tensor:
        """a buffer of `_denoise_tiled`, owned by the Denoiser (no engine has the image's shape), allocated on first use and grown on demand"""
        buf = self.__dict__.setdefault("_tile", {})
        if name not in buf or buf[name].numel() < numel:
            buf[name] = (torch.zeros((numel,), dtype=dtype).pin_memory() if pinned else torch.zeros((numel,), dtype=dtype, device=self.device))
        return buf[name]

    _TILE_HEAD = 16             # the byte buffer of a tiled image starts with SSDN_OP_NOISE_EST's tables: offs int64 [1], ext int32 [2]

    def _denoise_tiled(self, t: Tensor, T: int, O: int, value, kind: Optional[str], batch_size: int, std: bool,
                       white: Optional[int] = None) -> Dict:
        """One image larger than the tile, through the inference plan (B, T, T) in overlapping tiles (include/ssdn_hip.h, SSDN_OP_TILE_IN /
        SSDN_OP_TILE_OUT).  t: uint8 CPU tensor [h, w, C]; value: the noise parameter, None, or "auto" with `kind`
        the estimator's.  One pinned upload; per batch of at most `batch_size` tiles TILE_IN into the engine's input, the run, a device
        copy of its output into the tile store (with std also the posterior launch and a copy into a second store); then TILE_OUT, one
        download and one synchronisation.  A store is Kx Ky C T^2 4 bytes.  -> {"out", "tiles", ["noise_std"], ["std"], ["noise_param"]}.
        A uint16 t (never with "auto") stages its samples behind the same 16-byte head and runs SSDN_OP_TILE_IN16 / SSDN_OP_TILE_OUT16 at
        `white`; "out" is then uint16."""
        from ssdn.hip import lib as L
        from ssdn.hip import engine as E
        ssdn_pipe = self._pipeline == Pipeline.SSDN
        h, w, Cn = (int(v) for v in t.shape)
        Kx, Ky = L.tile_count(w, T, O), L.tile_count(h, T, O)
        n, nb, head, S = Kx * Ky, w * h * Cn, self._TILE_HEAD, T - O
        wide = t.dtype == torch.uint16
        size = 2 if wide else 1                              # bytes of a sample
        if nb >= 2 ** 31:
            raise ValueError("denoise: an image of %d x %d x %d is beyond the 2^31 %s the tile ops address"
                             % (w, h, Cn, "samples" if wide else "bytes"))
        host = self._tile_buffer("host_in", head + size * nb, torch.uint8, pinned=True)
        dev = self._tile_buffer("dev_in", head + size * nb, torch.uint8)
        host[:8].view(torch.int64)[0] = 0
        host[8:16].view(torch.int32).copy_(torch.tensor([w, h], dtype=torch.int32))
        host[head:head + size * nb].view(t.dtype)[:] = t.reshape(-1)
        dev[:head + size * nb].copy_(host[:head + size * nb], non_blocking=True)
        img = dev[head:head + size * nb].view(t.dtype)
        auto = isinstance(value, str)
        if auto:
            # one estimate over the whole image (B = 1, a tensor of the image's own extent): Denoiser.estimate_noise's, whatever the tiling
            hist = self._tile_buffer("est_hist", L.NOISE_EST_CLASSES * L.NOISE_EST_BINS, torch.int32)
            ssum = self._tile_buffer("est_ssum", L.NOISE_EST_CLASSES, torch.int64)
            est = self._tile_buffer("est", L.NOISE_EST_NEST, torch.float64)
            par = self._tile_buffer("est_param", 1, torch.float32)
            a = L.NoiseEstArgs(E._ptr(img), nb, E._ptr(dev), E._ptr(dev, 8), 1, Cn, w, h, L.NOISE_EST_KIND[kind], E._ptr(hist), E._ptr(ssum),
                               E._ptr(est), E._ptr(par))
            E.OpList([("noise_est", a)]).run(E.current_stream())
        store = self._tile_buffer("store", n * Cn * T * T, torch.float32)[:n * Cn * T * T].view(n, Cn, T, T)
        store_std = self._tile_buffer("store_std", n * Cn * T * T, torch.float32)[:n * Cn * T * T].view(n, Cn, T, T) if std else None
        nstd = []                                            # per tile: a 0-dim device tensor
        for k0 in range(0, n, batch_size):
            B = min(batch_size, n - k0)
            eng = self._engine(B, T, T, False)
            data = [E.tile_in(img, w, h, T, O, k0, eng.inp, white=white if wide else None)]
            if auto:                                         # broadcast on the device: no host round trip
                eng.noise_param.copy_(par[:1].expand(B))
                data += [torch.zeros(0), {NoisyDataset.Metadata.INPUT_NOISE_VALUES: eng.noise_param}]
            elif value is not None:
                data += [torch.zeros(0), {NoisyDataset.Metadata.INPUT_NOISE_VALUES: torch.full((B, 1, 1, 1), value)}]
            self._run(data, clone=False)                     # (no_grad: the inference plan, whose input is already in place)
            store[k0:k0 + B].copy_(eng.pme if ssdn_pipe else eng.main.tensor("out32"))
            if std:
                store_std[k0:k0 + B].copy_(eng.posterior(cov=False, std=True)["std"])
            if ssdn_pipe:
                for b in range(B):
                    if eng.style == "poisson":               # a map: over the part of the tile inside the image
                        ky, kx = divmod(k0 + b, Kx)
                        nstd.append(eng.noise_std[b, :min(T, w - kx * S), :min(T, h - ky * S)].mean())
                    else:
                        nstd.append(eng.noise_std[0 if self._const else b].clone())
        res: Dict = {"tiles": n}
        dev_out = self._tile_buffer("dev_out", size * nb, torch.uint8)[:size * nb].view(t.dtype)
        host_out = self._tile_buffer("host_out", size * nb, torch.uint8, pinned=True)[:size * nb].view(t.dtype)
        E.tile_out(store, w, h, T, O, 0, dev_out, white=white if wide else None)
        host_out[:nb].copy_(dev_out[:nb], non_blocking=True)
        if std:
            dev_std = self._tile_buffer("dev_std", nb, torch.float32)
            host_std = self._tile_buffer("host_std", nb, torch.float32, pinned=True)
            E.tile_out(store_std, w, h, T, O, 1, dev_std)
            host_std[:nb].copy_(dev_std[:nb], non_blocking=True)
        torch.cuda.current_stream().synchronize()
        res["out"] = host_out[:nb].view(h, w, Cn).clone()
        if std:
            res["std"] = host_std[:nb].view(Cn, h, w).clone()
        if ssdn_pipe:
            res["noise_std"] = float(torch.stack(nstd).cpu().to(torch.float64).mean())
        if auto:
            res["noise_param"] = float(par.cpu()[0])
        return res

    def denoise(self, images: List, noise_param=None, batch_size: int = 1, bucket: Optional[int] = None, uniform: bool = False,
                std: bool = False, tile: Optional[int] = None, overlap: Optional[int] = None, white: Optional[int] = None,
                risk: bool = False, risk_margin: int = 16) -> Dict:
        """Denoise already noisy images.  images: uint8 arrays or tensors [h, w] or [h, w, C], upright as PIL hands them out, of any and
        differing sizes, C the model's channel count.  Every image is reflection-padded bottom and right to a multiple of `bucket`
        (default and unit: NoiseNetwork.input_wh_mul(); larger values trade padding for fewer distinct plans -- at most _MAX_ENGINES are
        cached and one owns ~1 GB), to a square for a blind-spot model, with uniform=True to the largest image of the call (the
        evaluator's pad_uniform); images of one padded shape run in batches of at most `batch_size`, a short last batch at its own size.
        Per batch: one pinned upload of the packed bytes, SSDN_OP_IMAGE_IN (/ 255, transpose, pad), an inference run under no_grad
        whatever the module's mode, SSDN_OP_IMAGE_OUT (crop, clip, * 255, truncate, transpose), one download (csrc/image_io.hip, DESIGN.md
        section 3.16): the bytes `tensor2image` would give for the un-padded IMG_DENOISED of the same run.
        noise_param: required for an ssdn model with a known noise parameter, refused (ValueError, before any device work) for every
        other model; the numeric part of the noise style -- gauss: an integer is /255, poisson: lambda, impulse: an integer is per cent.
        "auto" (known gauss and poisson models; an impulse model refuses it: there is no estimator for impulse noise) estimates it per
        image on the device between SSDN_OP_IMAGE_IN and the run (`estimate_noise`) and adds "noise_param": the fp32 value used per
        image; an image too small or too saturated for an estimate raises ValueError naming its index.
        -> {"out": uint8 CPU tensors of the inputs' shapes, in input order}; ssdn models also "noise_std": per image the mean of
        NOISE_STD_DEV over its extent; std=True (ssdn only) adds "std": float32 [C, h, w] upright posterior std maps (Denoiser.posterior's).
        tile=T (a positive multiple of 32; overlap=O a multiple of 32 with 0 <= 2 O <= T, default T / 4 rounded down to a multiple of 32, at
        least 32 and at most T / 2 rounded down to one; overlap without tile and values outside these raise ValueError before any device
        work): an image with w <= T and h <= T takes the route above untouched, byte for byte (uniform=True then pads to the largest of
        THESE images); every other image is cut into T x T tiles whose origins are multiples of T - O, which run through ONE inference plan
        (B, T, T) in batches of at most batch_size tiles of that image and are blended linearly across the overlaps (SSDN_OP_TILE_IN /
        SSDN_OP_TILE_OUT, csrc/tile_io.hip, include/ssdn_hip.h for the definition); bucket and uniform do not apply
        to it.  Its bytes go up once into a buffer the Denoiser owns and come down once; between them the tiles' outputs wait in a store of
        Kx Ky C T^2 4 bytes on the device (~1 GB for 45 megapixels at T = 512, O = 128; std=True keeps a second one), allocated on first
        use and grown to the largest image.  "auto" estimates ONE parameter over the whole image -- `estimate_noise([image])`'s, bit for
        bit, whatever the tiling -- and every tile takes it.  "noise_std" of a tiled image is the float64 mean over its tiles of the
        per-tile value (poisson: of each tile's map over the part of the tile inside the image); a model that estimates the noise level
        from its input (a variable unknown noise level: the sigma network) does so per TILE, a known difference from a whole-image run.
        With tile the result gains "tiles": Kx Ky per image, 1 for an image that was not tiled.
        16-bit images (uint16 arrays or tensors; include/ssdn_hip.h, SSDN_OP_IMAGE_IN16): two bytes per sample
        cross the bus, the value is min(sample, white) / white and "out" is uint16 of the input's shape -- clipped, * white, rounded to
        nearest even.  white: the sample value that means 1.0, an integer in [1, 65535], None = 65535 (4095 for a 12-bit file); giving
        it to a call without a uint16 image is a ValueError.  Images group by (dtype, padded shape): a call may mix both depths, and its
        uint8 images come out exactly as from a call with only them.  A number as noise_param keeps its meaning (gauss 25: sigma =
        25 / 255 of white); "auto" with a uint16 image is a ValueError before any device work: the estimator is defined on bytes.
        risk=True (ssdn models with a gauss or poisson style; every other model raises NotImplementedError, as `risk` does) adds "risk":
        per image a dict of Python floats, ssdn.utils.risk_values' -- "psnr_out_est" and "psnr_mu_est" estimate the PSNR of "out" and of
        the prior mean against the clean image nobody has, "nll" is the negative log-likelihood of the noisy pixels under the model (see
        `risk` for the rest and for the caveats: clipping, padded borders, a wrong noise parameter) -- over the image's extent shrunk by
        risk_margin pixels on every side; an image of at most 2 risk_margin pixels in an axis has NaN values.  SSDN_OP_RISK runs between
        the inference run and SSDN_OP_IMAGE_OUT and its statistics are read behind the synchronisation the download already has: "out"
        is byte for byte what it is without the flag.  With "auto" the op reads the parameter the estimator wrote.  risk=True with tile=
        is a ValueError: overlapping tiles would count pixels twice.
        Like `posterior` it never becomes the forward that backward() / optimizer_step() / accumulate_metrics() act on."""
        ssdn_pipe = self._pipeline == Pipeline.SSDN
        if risk:
            self.check_risk("denoise: risk=True")
            if tile is not None:
                raise ValueError("denoise: risk=True with tile= is not supported: overlapping tiles would count pixels twice")
            risk_margin = int(risk_margin)
            if risk_margin < 0:
                raise ValueError("denoise: risk_margin must be at least 0, got %d" % risk_margin)
        value = self._noise_param_value(noise_param)
        tile, overlap = self._tile_options(tile, overlap)
        if std and not ssdn_pipe:
            raise ValueError("denoise: std=True needs a posterior: the %s pipeline has none (ssdn models only)" % self._pipeline.value)
        bucket, batch_size = self._denoise_options(bucket, batch_size)
        imgs = self._denoise_images(images)
        auto = isinstance(value, str)                    # "auto": the value is estimated per image on the device
        wide = [k for k, t in enumerate(imgs) if t.dtype == torch.uint16]
        if white is not None:
            from ssdn.hip.engine import check_white
            white = check_white(white, "denoise: white")
            if not wide:
                raise ValueError("denoise: white is the white level of uint16 images and this call has none")
        if auto and wide:
            raise ValueError("denoise: noise_param 'auto' with a 16-bit image (image %d): %s" % (wide[0], NOISE_EST_BYTES_ONLY))
        res: Dict = {"out": [None] * len(imgs)}
        if auto:
            from ssdn.utils import noise
            kind = noise.parse_style(self.cfg[ConfigValue.NOISE_STYLE])[0]
            res["noise_param"] = [None] * len(imgs)
        if ssdn_pipe:
            res["noise_std"] = [None] * len(imgs)
        if std:
            res["std"] = [None] * len(imgs)
        if tile is not None:
            res["tiles"] = [1] * len(imgs)
        if risk:
            res["risk"] = [None] * len(imgs)
        if not imgs:
            return res
        tiled = [k for k, t in enumerate(imgs) if tile is not None and (t.shape[1] > tile or t.shape[0] > tile)]
        whole = [k for k in range(len(imgs)) if k not in tiled]
        # by (dtype, padded shape): a batch is of one dtype, and `uniform` pads to the largest image of the same depth
        groups = {}
        for dt in (torch.uint8, torch.uint16):
            same = [k for k in whole if imgs[k].dtype == dt]
            if same:
                groups.update({(dt,) + hw: m for hw, m in self._denoise_groups(imgs, bucket, uniform, same).items()})
        keep = (self._last_engine, getattr(self, "_has_loss_last", None))
        try:
            with torch.no_grad():
                for k in tiled:
                    one = self._denoise_tiled(imgs[k], tile, overlap, value, kind if auto else None, batch_size, std, white)
                    if auto and not math.isfinite(one["noise_param"]):
                        raise ValueError("denoise: image %d has too few valid 3x3 windows for a noise estimate (it is smaller "
                                         "than 3x3 or saturated): pass noise_param as a number" % k)
                    one["out"] = one["out"] if images[k].ndim == 3 else one["out"][:, :, 0]
                    for name, v in one.items():
                        res[name][k] = v
                for (dt, H, W), members in groups.items():
                    for lo in range(0, len(members), batch_size):
                        idx = members[lo:lo + batch_size]
                        B = len(idx)
                        eng = self._engine(B, H, W, False)
                        data = [eng.image_in([imgs[k] for k in idx], white=white if dt == torch.uint16 else None)]
                        if auto:
                            # the estimates land in the engine's parameter tensor, which _run takes as it is: no host round trip
                            eng.estimate_noise(kind, into_noise_param=True)
                            data += [torch.zeros(0), {NoisyDataset.Metadata.INPUT_NOISE_VALUES: eng.noise_param}]
                        elif value is not None:
                            data += [torch.zeros(0), {NoisyDataset.Metadata.INPUT_NOISE_VALUES: torch.full((B, 1, 1, 1), value)}]
                        self._run(data, clone=False)         # (no_grad: the inference plan of this shape, whose input is already in place)
                        rstats = eng.risk(eng.image_extents(), risk_margin) if risk else None
                        outs = eng.image_out()
                        if risk:                             # (image_out has synchronised)
                            vals = ssdn.utils.risk_values(rstats.cpu(), eng.C)
                            for b, k in enumerate(idx):
                                res["risk"][k] = {name: float(v[b]) for name, v in vals.items()}
                        if auto:                             # (image_out has synchronised)
                            used = eng.noise_param.cpu()
                            for b, k in enumerate(idx):
                                if not math.isfinite(float(used[b])):
                                    raise ValueError("denoise: image %d has too few valid 3x3 windows for a noise estimate (it is smaller "
                                                     "than 3x3 or saturated): pass noise_param as a number" % k)
                                res["noise_param"][k] = float(used[b])
                        smap = eng.posterior(cov=False, std=True)["std"].cpu() if std else None
                        nstd = (eng.noise_std if eng.style == "poisson" else eng.noise_std.cpu()) if ssdn_pipe else None
                        for b, k in enumerate(idx):
                            h, w = imgs[k].shape[:2]
                            o = outs[b].clone()
                            res["out"][k] = o if images[k].ndim == 3 else o[:, :, 0]
                            if ssdn_pipe:
                                # gauss / impulse: one value per sample (a learnable scalar: one for all); poisson: a map
                                res["noise_std"][k] = (float(nstd[b, :w, :h].mean()) if eng.style == "poisson"
                                                       else float(nstd[0 if self._const else b]))
                            if std:
                                res["std"][k] = smap[b, :, :w, :h].permute(0, 2, 1).contiguous()
        finally:
            self._last_engine, self._has_loss_last = keep
        return res

    def backward(self):
        """Run the planned backward pass of the last training-mode run_pipeline; gradients land in `flat_grad` and are
        visible as `.grad` of every parameter."""
        eng = self._last_train_engine
        if eng is None or not eng.train:
            raise RuntimeError("backward() needs a preceding training-mode run_pipeline()")
        adds = self._adds()
        via_vjp = self._sync_accumulate(eng, adds)
        if not eng.loss_fwd or (eng.g_fresh and not via_vjp):
            eng.backward()
        else:       # an autograd backward of this forward has replaced the loss gradient: the VJP of mean(LOSS) restores it
            eng.vjp_backward(w=torch.full((eng.B,), 1.0 / eng.B, device=self.device))
        self._count_backward(adds)
        self._expose_grads()
        # this route consumes the forward: its IMG_DENOISED / IMG_MU leave the graph, as they were before autograd reached them, so code
        # written for the planned backward (run_pipeline, backward(), then numpy on the images) keeps working
        g = self._img_graph
        if g is not None and g[0] is eng and g[1] == eng.gen:
            for r in g[2]:
                t = r()
                if t is not None and t.grad_fn is not None:
                    t.detach_()
            self._img_graph = None

    def _backward_engine(self, eng, w: Optional[Tensor] = None, g_pme: Optional[Tensor] = None, g_mu: Optional[Tensor] = None,
                         want_dx: bool = False):
        if eng is None or not eng.train:
            raise RuntimeError("this output was not produced by a training-mode run_pipeline()")
        adds = self._adds()
        self._sync_accumulate(eng, adds)
        eng.vjp_backward(w, g_pme, g_mu, want_dx=want_dx)
        self._count_backward(adds)
        self._expose_grads()

    def _expose_grads(self):
        for net, base in ((self._models[Denoiser.MODEL], 0),) + (((self._models[Denoiser.SIGMA_ESTIMATOR], self._n_main),) if self._var else ()):
            for l in net.layers:
                h = net.get_submodule(l.name)
                h.weight.grad = self.flat_grad[base + l.w_off: base + l.w_off + l.M * l.cin * l.k * l.k].view(l.M, l.cin, l.k, l.k)
                h.bias.grad = self.flat_grad[base + l.b_off: base + l.b_off + l.M]
        if self._const:
            o = self._n_main + self._n_sig
            self.l_params[Denoiser.ESTIMATED_SIGMA].grad = self.flat_grad[o:o + 1].view(1, 1, 1, 1)
        self._grads_exposed = True

    def optimizer_step(self, lr: float, grad_scale: float = 1.0):
        """Fused Adam (betas 0.9/0.99, eps 1e-8; train.py:100-107) over the flat buffer + re-pack of the fp16 MFMA shadows.
        Acts on the engine of the last TRAINING-mode run_pipeline (an eval / snapshot call in between does not matter)."""
        eng = self._last_train_engine
        if eng is None:
            raise RuntimeError("optimizer_step() needs a preceding training-mode run_pipeline()")
        self.adam_steps += 1
        eng.adam(lr, self.adam_steps, grad_scale)
        self._grad_terms = 0                 # the sum is spent: the next backward overwrites
        # the kernel wrote the flat buffer through a raw pointer: bump our own counter (torch's did not move); the shadows of
        # THIS engine are fresh, other cached shapes and the nets' own forward engines re-pack lazily
        self.mark_dirty()
        for slot in self._engines.values():
            if slot[0] is eng:
                slot[1] = self._param_version()

    def gradient_exchange(self, world: int):
        """The bucketed, backward-overlapped all-reduce of this model's flat gradient (ssdn.hip.dp.GradExchange)."""
        from ssdn.hip import dp
        net = self._models[Denoiser.MODEL]
        return dp.GradExchange(world, dp.bucket_ranges(net.layers, self._n_main, self.flat.numel()), self.device)

    # ---- H11: per-step metrics on the device ---------------------------------------------------------------------------
    METRIC_NAMES = ("loss", "psnr_out", "psnr_mu_out", PipelineOutput.NOISE_STD_DEV.value, PipelineOutput.MODEL_STD_DEV.value)
    assert len(METRIC_NAMES) <= 7       # the accumulator is 16 floats: (sum, count) per metric in [0, 14), the kernel's arrival counter in [15]

    def _metrics_acc(self, kind: str) -> Tensor:
        accs = self.__dict__.setdefault("_macc", {})
        if kind not in accs:
            accs[kind] = torch.zeros(16, dtype=torch.float32, device=self.device)
        return accs[kind]

    def _clean_and_extent(self, meta: Dict):
        """The clean batch of a pipeline's metadata as the device kernels read it, and the un-padded extents of its samples:
        -> (clean: contiguous fp32 [B,C,H,W] on the device; ext: int32 [B,2] on the device, or None when no sample is padded;
        the extents on the host, int32 [B,2], or None without Metadata.IMAGE_SHAPE)."""
        MD = NoisyDataset.Metadata
        clean = meta[MD.CLEAN]
        B = clean.shape[0]
        if clean.device != self.device or clean.dtype != torch.float32 or not clean.is_contiguous():
            clean = clean.to(self.device, torch.float32, non_blocking=True).contiguous()
        ext = None
        shp = meta.get(MD.IMAGE_SHAPE)
        if shp is not None:
            shp = torch.as_tensor(shp).reshape(B, -1)[:, -2:].to(torch.int32)
            if bool((shp != torch.tensor(list(clean.shape[-2:]), dtype=torch.int32)).any()):
                ext = shp.to(self.device, non_blocking=True).contiguous()
        return clean, ext, shp

    def accumulate_metrics(self, data: List, kind: str = "train", with_loss: bool = True, per_sample: bool = False):
        """Add the metrics of the LAST `run_pipeline` / `train_step` batch (`data` = its inputs) to the device-resident accumulator
        `kind` with one kernel launch (SSDN_OP_METRICS: loss, PSNR of IMG_DENOISED and IMG_MU against the clean image over each
        sample's un-padded extent, noise / model std-dev x 255 -- what the reference trainer accumulates with ~20 ATen launches per
        step, train.py:205-218, utils/data.py:94-105).  Nothing is copied to the host; `read_metrics` does that when the trainer
        prints.  per_sample=True returns {"psnr_out": [B], "psnr_mu_out": [B]} of this batch (host tensors: synchronises).
        A batch whose metadata has no Metadata.CLEAN (images that are already noisy) adds its loss and std-dev sums only: no PSNR sum or
        count moves."""
        eng = self._last_engine
        if eng is None:
            raise RuntimeError("accumulate_metrics() needs a preceding run_pipeline()")
        meta = data[NoisyDataset.METADATA]
        if not torch.is_tensor(meta.get(NoisyDataset.Metadata.CLEAN)):
            # a batch of images that are already noisy (ssdn.datasets.DevicePoolStream): loss and the std-dev metrics only, no PSNR sum moves
            if per_sample:
                raise ValueError("accumulate_metrics(): the batch has no clean image (Metadata.CLEAN): there is no per-sample PSNR")
            eng.accumulate_metrics(self._metrics_acc(kind), None, None, with_loss=with_loss and self._has_loss_last)
            return None
        clean, ext, _ = self._clean_and_extent(meta)
        eng.accumulate_metrics(self._metrics_acc(kind), clean, ext, with_loss=with_loss and self._has_loss_last)
        self._metrics_keep = (clean, ext)               # alive until the launch has run
        if per_sample:
            per = eng.metrics_per.cpu()                      # (synchronises: the launch has run)
            if kind != "train":
                self._metrics_acc(kind).zero_()              # only the per-sample values of such a batch are used: its sums must not pile up
            res = {"psnr_out": per[:, 1].clone()}
            if self._pipeline == Pipeline.SSDN:
                res["psnr_mu_out"] = per[:, 2].clone()
            return res
        return None

    def ssim(self, data: List, maps: bool = False) -> Dict[str, Tensor]:
        """SSIM against the clean image for the LAST `run_pipeline` / `train_step` batch (`data` = its inputs), per sample over its
        un-padded extent (ssdn.utils.calculate_ssim is the definition).  -> host float32 [B] tensors "ssim_nsy" (the noisy input),
        "ssim_out" (IMG_DENOISED) and, for the SSDN pipeline, "ssim_mu_out" (IMG_MU); maps=True adds "map_nsy", "map_out"
        ("map_mu_out"): [B,C,H,W], the value of every 11 x 11 window at its centre, zero where none is centred.  On a GPU the engine's
        own buffers go through SSDN_OP_SSIM (csrc/ssim.hip: fp64 window sums, one rounding); a Denoiser on another device has no
        engine and no last batch.  Reads only: outputs, metric accumulators, weights and plans stay what they were.  Synchronises."""
        eng = self._last_engine
        if eng is None:
            raise RuntimeError("ssim() needs a preceding run_pipeline()")
        meta = data[NoisyDataset.METADATA] if len(data) > NoisyDataset.METADATA else None
        if not isinstance(meta, dict) or not torch.is_tensor(meta.get(NoisyDataset.Metadata.CLEAN)):
            raise ValueError("ssim(): the batch has no clean image (Metadata.CLEAN)")
        clean, ext, shp = self._clean_and_extent(meta)
        if tuple(clean.shape) != (eng.B, eng.C, eng.H, eng.W):
            raise ValueError("ssim(): the clean batch %s is not the last run's shape" % (tuple(clean.shape),))
        small = min(clean.shape[-2:]) if shp is None else int(shp.min())
        if small < 11:
            raise ValueError("ssim(): an image extent of %d is below the 11 x 11 window" % small)
        srcs = [("nsy", eng.inp), ("out", eng.pme if self._pipeline == Pipeline.SSDN else eng.main.tensor("out32"))]
        if self._pipeline == Pipeline.SSDN:
            srcs.append(("mu_out", eng.mu))
        res = {}
        for name, x in srcs:
            val, smap = eng.ssim(x, clean, ext, want_map=maps)
            res["ssim_" + name] = val.cpu()                      # (synchronises: the launch has run, the buffers are free for the next)
            if maps:
                res["map_" + name] = smap.cpu()
        return res

    def calibration(self, data: List, hist: bool = False, maps: bool = False) -> Dict[str, Tensor]:
        """Calibration of the per-pixel posterior N(IMG_DENOISED, cov) against the clean image for the LAST `run_pipeline` / `train_step`
        batch (`data` = its inputs), per sample over its un-padded extent (ssdn.utils.calculate_calibration is the definition).  -> host
        float64 [B] tensors "nll" (nats per pixel-channel), "maha" (mean squared Mahalanobis distance per channel: ideal 1, above 1 the
        model is over-confident), "rmse_ratio" (actual over predicted RMSE), "cover_1s" / "cover_2s" / "cover_3s" (share of |z_c| <= 1, 2,
        3; nominal 0.6827, 0.9545, 0.9973), "cover_50" / "cover_90" / "cover_99" (share of pixels inside the chi^2_C region of that
        level), "degenerate" (share of pixels whose covariance is not positive definite or not finite: left out of the rest), and the raw
        "stats" [B,12].  hist=True adds "hist", int64 [B,C,34] (z_c in 32 bins of width 0.25 over [-4, 4) and the two tails); maps=True
        adds "zmap" [B,C,H,W], NaN at degenerate pixels and outside the extents.  For an impulse model the posterior is a two-component
        mixture and cov its moment-matched covariance (see `posterior`): the values describe that Gaussian.  On a GPU one
        SSDN_OP_HEAD_POSTERIOR and one SSDN_OP_CALIBRATION launch behind the last forward (csrc/calibration.hip: fp64 per pixel); a
        Denoiser on another device has no engine and no last batch.  Reads only: outputs, metric accumulators, weights, plans and the
        last engines stay what they were.  Synchronises.  SSDN pipeline only."""
        if self._pipeline != Pipeline.SSDN:
            raise NotImplementedError("Denoiser.calibration: the %s pipeline has no posterior covariance (SSDN pipeline only)" % self._pipeline.value)
        eng = self._last_engine
        if eng is None:
            raise RuntimeError("calibration() needs a preceding run_pipeline()")
        meta = data[NoisyDataset.METADATA] if len(data) > NoisyDataset.METADATA else None
        if not isinstance(meta, dict) or not torch.is_tensor(meta.get(NoisyDataset.Metadata.CLEAN)):
            raise ValueError("calibration(): the batch has no clean image (Metadata.CLEAN)")
        clean, ext, _ = self._clean_and_extent(meta)
        if tuple(clean.shape) != (eng.B, eng.C, eng.H, eng.W):
            raise ValueError("calibration(): the clean batch %s is not the last run's shape" % (tuple(clean.shape),))
        stats, dhist, dmap = eng.calibration(clean, ext, want_hist=hist, want_map=maps)
        stats = stats.cpu()                                      # (synchronises: the launches have run, the buffers are free for the next)
        res = dict(ssdn.utils.calibration_values(stats, eng.C))
        res["stats"] = stats
        if hist:
            res["hist"] = dhist.cpu()
        if maps:
            res["zmap"] = dmap.cpu()
        return res

    def check_risk(self, who: str = "Denoiser.risk") -> None:
        """Raise NotImplementedError unless this model has the reference-free risk estimate (`risk`): the SSDN pipeline with a gauss or
        poisson noise style.  Decided from the configuration alone, before any device work."""
        if self._pipeline != Pipeline.SSDN:
            raise NotImplementedError("%s: the %s pipeline has no reference-free risk estimate (SSDN pipeline only): ssdn_u_only has no "
                                      "head and so no noise variance, and the output of an MSE pipeline depends on the pixel itself, so it "
                                      "would need a divergence estimate" % (who, self._pipeline.value))
        from ssdn.utils import noise
        kind = noise.parse_style(self.cfg[ConfigValue.NOISE_STYLE])[0]
        if kind not in ("gauss", "poisson"):
            raise NotImplementedError("%s: no reference-free risk estimate for an %s model: its posterior mean is not affine in the pixel "
                                      "and its noise is not zero-mean (gauss and poisson models only)" % (who, kind))

    def risk(self, data: List, margin: int = 16) -> Dict[str, Tensor]:
        """A reference-free estimate of the error of the LAST `run_pipeline` / `train_step` batch (`data` = its inputs), per sample over
        its un-padded extent shrunk by `margin` pixels on all four sides -- no clean image is read (ssdn.utils.calculate_risk is the
        definition, ssdn.utils.risk_values the reported values).  -> host float64 [B] tensors "mse_mu_est" / "mse_out_est" (unbiased
        estimates of the mean squared error of IMG_MU and IMG_DENOISED against the clean image), "psnr_mu_est" / "psnr_out_est" (NaN where
        the estimate is <= 0: it is unbiased, not positive), "mse_mu_se" / "mse_out_se" (naive standard errors), "nll" (nats per
        pixel-channel of the NOISY image under the model's marginal), "weight" (how much of its own noisy value a pixel's output keeps),
        "clipped" (share of samples at or beyond 0 / 1, where the noise is not zero-mean), "degenerate", and the raw "stats" [B,12].  The
        extent comes from the batch's metadata (Metadata.IMAGE_SHAPE), or is the whole image when there is none.  margin: a pixel near a
        reflection-padded edge has a copy of itself inside the network's field of view, so the estimate is optimistic there; an extent of
        at most 2 margin in an axis has N = 0 and NaN values.  The estimate inherits an error of the noise parameter given to a
        known-noise model: a sigma that is too large reads as a better PSNR.  On a GPU two launches behind the last forward
        (SSDN_OP_RISK, csrc/risk.hip: fp64 per pixel).  Reads only: outputs, metric accumulators, weights, plans and the last engines
        stay what they were.  Synchronises.  SSDN pipeline with a gauss or poisson style (every NOISE_VALUE mode, full and diagonal
        covariance); every other model raises NotImplementedError."""
        self.check_risk()
        margin = int(margin)
        if margin < 0:
            raise ValueError("risk(): margin must be at least 0, got %d" % margin)
        eng = self._last_engine
        if eng is None:
            raise RuntimeError("risk() needs a preceding run_pipeline()")
        meta = data[NoisyDataset.METADATA] if len(data) > NoisyDataset.METADATA else None
        ext = None
        shp = meta.get(NoisyDataset.Metadata.IMAGE_SHAPE) if isinstance(meta, dict) else None
        if shp is not None:
            shp = torch.as_tensor(shp).reshape(eng.B, -1)[:, -2:].to(torch.int32)
            ext = shp.to(self.device).contiguous()
        stats = eng.risk(ext, margin).cpu()                      # (synchronises: the launches have run, the buffers are free for the next)
        res = dict(ssdn.utils.risk_values(stats, eng.C))
        res["stats"] = stats
        return res

    def reset_device_metrics(self, kind: str = "train"):
        """forget what `accumulate_metrics` has summed on the device since the last read (the trainer's reset_metrics)"""
        if kind in self.__dict__.get("_macc", {}):
            self._macc[kind].zero_()

    def read_metrics(self, kind: str = "train", reset: bool = True) -> Dict[str, Tuple[float, int]]:
        """{metric name: (sum over samples, sample count)} accumulated since the last reset -- ONE 64-byte copy to the host."""
        acc = self._metrics_acc(kind)
        v = acc.cpu().tolist()
        if reset:
            acc.zero_()
        return {name: (v[2 * k], int(round(v[2 * k + 1]))) for k, name in enumerate(self.METRIC_NAMES) if v[2 * k + 1] > 0}

    def train_step(self, data: List, lr: float, exchange=None, metrics: bool = False) -> Dict:
        """One whole optimisation step on this GPU: forward + loss + backward + Adam.  exchange: `gradient_exchange(world)`
        for data parallelism -- the per-bucket all-reduces are issued behind events recorded inside the backward list, so
        they overlap the rest of the backward pass; Adam waits for them and folds in 1 / world.
        Behind n `accumulate_step` calls it adds its own micro-batch to their sum, exchanges that sum (the marks exist in this pass only)
        and steps Adam once with gscale = 1 / ((n + 1) * world): the update of the mean loss over the n + 1 micro-batches."""
        from ssdn.hip import dp
        out = self._run(data, clone=False, bridge=False, accumulate=True)
        eng = self._last_train_engine
        n = self._grad_terms if eng.accumulate else 0
        if metrics:                         # (reads the forward pass's outputs: enqueued in front of the backward pass)
            self.accumulate_metrics(data, "train")
        from ssdn.hip import engine as _engine
        scale = dp.exchange_step(lambda ex: eng.backward(exchange=ex, defer_tail=ex is None and _engine.DEFER_TAIL), self.flat_grad, exchange)
        self.optimizer_step(lr, scale if n == 0 else 1.0 / ((n + 1) * (exchange.world if exchange is not None else 1)))
        return out

    def accumulate_step(self, data: List, metrics: bool = False) -> Dict:
        """One micro-batch of a larger optimisation step: forward + loss + backward, the gradient ADDED to what the micro-batches since the
        last optimiser step left in `flat_grad` (the first one overwrites).  No gradient exchange, no optimiser step, no re-pack of the
        weight shadows: the `train_step` that closes the group does those once.  Returns what `train_step` returns."""
        out = self._run(data, clone=False, bridge=False, accumulate=True)
        eng = self._last_train_engine
        if metrics:
            self.accumulate_metrics(data, "train")
        n = self._grad_terms if eng.accumulate else 0
        eng.backward(defer_tail=False)       # (deferred reductions would read slabs that the next micro-batch overwrites)
        self._grad_terms = n + 1
        return out

    # ---- optimiser state in the reference's torch.optim.Adam layout (train.py:725,744: `.training` checkpoints) ----------
    def _param_slices(self):
        """(flat offset, numel, shape) of every parameter in `self.parameters()` order == the reference's order (the module
        tree mirrors it, incl. output_conv registered before output_block and the de-duplicated `_models` aliases)."""
        base = self.flat.data_ptr()
        res = []
        for p in self.parameters():
            off = (p.data_ptr() - base) // 4
            res.append((off, p.numel(), tuple(p.shape)))
        return res

    def optimizer_state_dict(self, lr: float = 3e-4) -> Dict:
        """State of the fused Adam as `torch.optim.Adam(denoiser.parameters(), betas=[0.9, 0.99]).state_dict()` would have it."""
        state = {}
        sl = self._param_slices()
        if self.adam_steps > 0:
            for i, (off, n, shape) in enumerate(sl):
                state[i] = {"step": torch.tensor(float(self.adam_steps)),
                            "exp_avg": self.adam_m[off:off + n].view(shape).clone(),
                            "exp_avg_sq": self.adam_v[off:off + n].view(shape).clone()}
        group = {"lr": lr, "betas": (0.9, 0.99), "eps": 1e-8, "weight_decay": 0, "amsgrad": False, "maximize": False,
                 "foreach": None, "capturable": False, "differentiable": False, "fused": None, "params": list(range(len(sl)))}
        return {"state": state, "param_groups": [group]}

    def load_optimizer_state_dict(self, sd: Dict):
        sl = self._param_slices()
        self.adam_m.zero_()
        self.adam_v.zero_()
        steps = 0
        for i, (off, n, shape) in enumerate(sl):
            st = sd.get("state", {}).get(i)
            if st is None:
                continue
            self.adam_m[off:off + n].copy_(st["exp_avg"].reshape(-1).to(self.adam_m))
            self.adam_v[off:off + n].copy_(st["exp_avg_sq"].reshape(-1).to(self.adam_v))
            steps = max(steps, int(float(st["step"])))
        self.adam_steps = steps
