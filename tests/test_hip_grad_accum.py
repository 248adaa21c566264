"""GPU: gradient accumulation over micro-batches.

The definition every test here pins: after passes 1..K into a clean buffer the flat gradient is fl(..fl(fl(g_1 + g_2) + g_3).. + g_K)
element by element, g_k being bit for bit what pass k writes in overwrite mode.  Every kernel involved is bit-reproducible and an fp32
`torch.add` on the device is the same IEEE operation as the epilogue's add, so the comparisons are `torch.equal`, no tolerance."""
import glob
import itertools
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from test_hip_denoiser_autograd import batch, seeded_denoiser
from test_hip_diag_cov import diag_denoiser
from test_hip_dp import _inputs, _make, _steps

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
K = 3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# ---- 4. op level ---------------------------------------------------------------------------------------------------------------------
class _Red:
    """one SSDN_OP_WREDUCE on random slabs: its argument struct and the tensors it points to"""

    def __init__(self, seed, nslabs, tapblock, with_bias, c_off, inv, m_off=0):
        from ssdn.hip import lib as L
        g = torch.Generator().manual_seed(seed)
        if tapblock:
            ntaps, M, Mpad, Kpad, cin = 3, 20, 32, 16, 40          # "taps" = channel blocks of a 1x1 layer: channel t * Kpad + k < cin
        else:
            ntaps, M, Mpad, Kpad, cin = 9, 20, 32, 16, 12
        cin_full = c_off + cin + 4
        self.slab0 = torch.randn(nslabs, ntaps, Mpad, Kpad, generator=g).to(DEV)
        self.bslab = torch.randn(nslabs, Mpad, generator=g).to(DEV)
        self.slab = self.slab0.clone()
        nw = (m_off + M) * cin_full * (1 if tapblock else ntaps)
        self.P_w = torch.randn(nw, generator=g).to(DEV)
        self.P_b = torch.randn(m_off + M, generator=g).to(DEV)
        self.gw, self.gb = self.P_w.clone(), self.P_b.clone()
        self.inv = torch.tensor([inv], dtype=torch.float32, device=DEV) if inv is not None else None
        self.with_bias = with_bias
        self.args = L.WreduceArgs(self.slab.data_ptr(), self.bslab.data_ptr(), nslabs, ntaps, M, Mpad, Kpad, cin, cin_full, m_off, c_off,
                                  int(tapblock), self.gw.data_ptr(), self.gb.data_ptr() if with_bias else None,
                                  self.inv.data_ptr() if self.inv is not None else None)

    def reset(self, fill, accumulate):
        """fresh slabs (stage 1 uses the slab buffer as scratch); gw / gb = NaN (to see what a pass writes) or the pre-fill P"""
        self.slab.copy_(self.slab0)
        if fill == "nan":
            self.gw.fill_(float("nan"))
            self.gb.fill_(float("nan"))
        else:
            self.gw.copy_(self.P_w)
            self.gb.copy_(self.P_b)
        self.args.accumulate = int(accumulate)

    def check(self, R_w, R_b):
        for out, P, R in ((self.gw, self.P_w, R_w), (self.gb, self.P_b, R_b)):
            written = ~torch.isnan(R)
            assert torch.equal(out[written], P[written] + R[written])
            assert torch.equal(out[~written], P[~written])                  # padding / a NULL gb: untouched
        assert (~torch.isnan(R_w)).sum() > 0 and bool((~torch.isnan(R_b)).any()) == self.with_bias


def _run_reductions(items):
    from ssdn.hip.engine import OpList, current_stream
    OpList([("wreduce", it.args) for it in items]).run(current_stream())      # (a run of consecutive reductions is ONE merged launch pair)
    torch.cuda.synchronize()


CASES = list(itertools.product((8, 70), (0, 1), (False, True), (0, 12), (None, 0.3)))


@pytest.mark.parametrize("inv", [None, 0.3])
def test_wreduce_accumulate_single_launch(inv):
    """gw / gb pre-filled with P: accumulate = 1 leaves fl(P + R), R the accumulate = 0 result of the same slabs (0.3: an FMA of the
    scale into the add would round differently), and touches nothing else.  nslabs <= 32 and > 32, tapblock, gb NULL, c_off > 0."""
    for i, (nslabs, tapblock, with_bias, c_off, inv_) in enumerate(CASES):
        if inv_ != inv:
            continue
        it = _Red(100 + i, nslabs, tapblock, with_bias, c_off, inv, m_off=4 if i % 3 == 0 else 0)
        it.reset("nan", 0)
        _run_reductions([it])
        R_w, R_b = it.gw.clone(), it.gb.clone()
        it.reset("P", 0)
        _run_reductions([it])                                                     # accumulate = 0 on a pre-filled buffer: overwrites, as before
        w = ~torch.isnan(R_w)
        assert torch.equal(it.gw[w], R_w[w]) and torch.equal(it.gw[~w], it.P_w[~w])
        it.reset("P", 1)
        _run_reductions([it])
        it.check(R_w, R_b)


@pytest.mark.parametrize("inv", [None, 0.3])
def test_wreduce_accumulate_merged_run(inv):
    """the same through k_wreduce_partial_multi + k_wreduce_multi: a run of five entries, the flag per entry of the table (mixed)"""
    cfgs = [(8, 0, True, 0), (70, 1, False, 12), (40, 0, True, 12), (70, 0, False, 0), (8, 1, True, 0)]
    items = [_Red(200 + i, ns, tb, wb, co, inv) for i, (ns, tb, wb, co) in enumerate(cfgs)]
    for it in items:
        it.reset("nan", 0)
    _run_reductions(items)
    R = [(it.gw.clone(), it.gb.clone()) for it in items]
    for it in items:
        it.reset("P", 1)
    _run_reductions(items)
    for it, (R_w, R_b) in zip(items, R):
        it.check(R_w, R_b)
    # mixed flags in one table: entries 1 and 3 overwrite, the others add
    for i, it in enumerate(items):
        it.reset("P", i % 2 == 0)
    _run_reductions(items)
    for i, (it, (R_w, R_b)) in enumerate(zip(items, R)):
        if i % 2 == 0:
            it.check(R_w, R_b)
        else:
            w = ~torch.isnan(R_w)
            assert torch.equal(it.gw[w], R_w[w]) and torch.equal(it.gw[~w], it.P_w[~w])
    # ... and the merged launch equals the single launches, entry by entry
    for it, (R_w, R_b) in zip(items, R):
        it.reset("nan", 0)
        _run_reductions([it])
        assert torch.equal(torch.nan_to_num(it.gw, nan=7.0), torch.nan_to_num(R_w, nan=7.0))


def test_accum_op_adds_once():
    from ssdn.hip import lib as L
    from ssdn.hip.engine import OpList, current_stream
    dst = torch.tensor([0.1, 1e8, -3.0, 5.0], device=DEV)
    src = torch.tensor([0.2, 1.0, 3.0, float("nan")], device=DEV)
    want = dst[:3] + src[:3]
    OpList([("accum", L.AccumArgs(dst.data_ptr(), src.data_ptr(), 3))]).run(current_stream())
    torch.cuda.synchronize()
    assert torch.equal(dst[:3], want) and float(dst[3]) == 5.0


# ---- 5. the definition, end to end -----------------------------------------------------------------------------------------------------
CONFIGS = [("ssdn", "gauss25", "known", 3, False), ("ssdn", "gauss25", "var", 3, False), ("ssdn", "gauss25", "const", 3, False),
           ("ssdn", "poisson30", "const", 3, False), ("ssdn", "gauss25", "known", 3, True), ("n2v", "gauss25", "known", 3, False),
           ("n2c", "gauss25", "known", 1, False)]


def _denoiser(alg, style, mode, ch, diag):
    return diag_denoiser(style, mode, ch) if diag else seeded_denoiser(alg, style, mode, ch)


def _chain(gs):
    s = gs[0].clone()
    for g in gs[1:]:
        s = s + g
    return s


def _upstream(out):
    from ssdn.params import PipelineOutput
    return 0.37 * out[PipelineOutput.LOSS].sum() + (out[PipelineOutput.IMG_DENOISED] ** 2).mean()      # NOT mean(LOSS)


@pytest.mark.parametrize("alg,style,mode,ch,diag", CONFIGS)
def test_accumulated_gradient_is_the_ordered_fp32_sum(alg, style, mode, ch, diag):
    d = _denoiser(alg, style, mode, ch, diag)
    data = [batch(alg, style, ch, 4, 64, seed=10 * k) for k in range(K)]
    assert not d.accumulate_grads and d._grad_terms == 0
    # the planned route
    gs = []
    for k in range(K):
        d.run_pipeline(data[k])
        d.backward()
        gs.append(d.flat_grad.clone())
    assert d._grad_terms == 0                       # overwriting passes do not count
    assert all(torch.isfinite(g).all() for g in gs) and not torch.equal(gs[0], gs[1]) and float(gs[0].abs().max()) > 0
    want = _chain(gs)
    d.zero_grad()
    for k in range(K):
        d.accumulate_step(data[k])
        assert d._grad_terms == k + 1
    torch.cuda.synchronize()
    assert torch.equal(d.flat_grad, want)           # (the whole buffer, padding tail included)
    d.accumulate_grads = True
    d.zero_grad()
    for k in range(K):
        d.run_pipeline(data[k])
        d.backward()
    assert torch.equal(d.flat_grad, want) and d._grad_terms == K
    d.zero_grad()
    d.run_pipeline(data[1])
    d.backward()
    assert torch.equal(d.flat_grad, gs[1])          # a clean buffer: the first pass overwrites
    # the autograd route, with an upstream gradient that is not mean(LOSS): in mode const the VJP's g_est must REPLACE the forward's
    d.accumulate_grads = False
    ga = []
    for k in range(K):
        _upstream(d.run_pipeline(data[k])).backward()
        ga.append(d.flat_grad.clone())
    assert not torch.equal(ga[0], gs[0])
    d.accumulate_grads = True
    d.zero_grad()
    for k in range(K):
        _upstream(d.run_pipeline(data[k])).backward()
    assert torch.equal(d.flat_grad, _chain(ga))
    for p in d.parameters():                        # .grad of every parameter is still a view of the flat buffer
        assert p.grad is not None and d.flat_grad.data_ptr() <= p.grad.data_ptr() < d.flat_grad.data_ptr() + 4 * d.flat_grad.numel()


# ---- 6. clean start ----------------------------------------------------------------------------------------------------------------------
def _planned(d, data):
    d.run_pipeline(data)
    d.backward()
    return d.flat_grad.clone()


@pytest.mark.parametrize("mode", ["known", "const"])
def test_clean_start_never_reads_stale_values(mode):
    d = seeded_denoiser("ssdn", "gauss25", mode, 3)
    data = [batch("ssdn", "gauss25", 3, 4, 64, seed=10 * k) for k in range(2)]
    g1, g2 = _planned(d, data[0]), _planned(d, data[1])
    # accumulate_grads = False (the default): two backward calls leave the second gradient alone
    assert torch.equal(d.flat_grad, g2) and not torch.equal(g1, g2)
    d.accumulate_grads = True
    d.flat_grad.fill_(float("nan"))
    d.zero_grad()
    assert torch.equal(_planned(d, data[0]), g1)
    assert torch.equal(_planned(d, data[1]), g1 + g2)
    # after optimizer_step(): whatever the buffer holds is not read (the padding floats have no writer: they are left alone here)
    d.optimizer_step(3e-4, 0.5)
    assert d._grad_terms == 0
    n_tot = d._n_main + d._n_sig + (1 if mode == "const" else 0)
    d.flat_grad[:n_tot].fill_(float("nan"))
    a = _planned(d, data[0])
    d.accumulate_grads = False
    b = _planned(d, data[0])                        # (an overwriting pass, by definition)
    assert torch.isfinite(a).all() and torch.equal(a, b)


@pytest.mark.parametrize("mode", ["known", "const"])
def test_torch_optimiser_sees_the_sum_of_two_losses(mode):
    from ssdn.params import PipelineOutput
    data = [batch("ssdn", "gauss25", 3, 4, 64, seed=10 * k) for k in range(3)]
    d = seeded_denoiser("ssdn", "gauss25", mode, 3)
    d.accumulate_grads = True
    opt = torch.optim.Adam(d.parameters(), lr=3e-4, betas=(0.9, 0.99))
    for k in range(2):                              # two losses through two backward calls
        d.run_pipeline(data[k])[PipelineOutput.LOSS].mean().backward()
    opt.step()
    # twin: the two gradients collected separately (overwrite mode), summed by torch
    t = seeded_denoiser("ssdn", "gauss25", mode, 3)
    topt = torch.optim.Adam(t.parameters(), lr=3e-4, betas=(0.9, 0.99))
    gs = []
    for k in range(2):
        t.run_pipeline(data[k])[PipelineOutput.LOSS].mean().backward()
        gs.append(t.flat_grad.clone())
    t.flat_grad.copy_(gs[0] + gs[1])                # (the parameters' .grad are views of it)
    topt.step()
    torch.cuda.synchronize()
    assert torch.equal(d.flat, t.flat) and not torch.equal(d.flat, seeded_denoiser("ssdn", "gauss25", mode, 3).flat)
    # the optimiser's zero_grad never reaches the module: set_to_none=True drops the handles, the buffer keeps the old sum
    for set_to_none, k in ((True, 2), (False, 0)):
        opt.zero_grad(set_to_none=set_to_none)
        d.run_pipeline(data[k])[PipelineOutput.LOSS].mean().backward()
        t.run_pipeline(data[k])[PipelineOutput.LOSS].mean().backward()     # (the twin overwrites)
        assert torch.equal(d.flat_grad, t.flat_grad), set_to_none


# ---- 7. the optimiser step -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,sizes", [("known", (4, 4, 4)), ("const", (4, 4, 4)), ("known", (4, 2)), ("var", (4, 2))])
def test_group_step_equals_adam_on_the_summed_gradient(mode, sizes):
    from ssdn.denoiser import Denoiser
    from ssdn.params import PipelineOutput
    n = len(sizes)
    data = [batch("ssdn", "gauss25", 3, b, 64, seed=10 * k) for k, b in enumerate(sizes)]
    lr = 3e-4
    d = seeded_denoiser("ssdn", "gauss25", mode, 3)
    for k in range(n - 1):
        d.accumulate_step(data[k])
    d.train_step(data[n - 1], lr)
    assert d.adam_steps == 1 and d._grad_terms == 0
    t = seeded_denoiser("ssdn", "gauss25", mode, 3)
    gs = [_planned(t, data[k]) for k in range(n)]
    t.flat_grad.copy_(_chain(gs))
    t.adam_steps += 1
    t._last_train_engine.adam(lr, t.adam_steps, gscale=1.0 / n)
    torch.cuda.synchronize()
    assert torch.equal(d.flat, t.flat) and torch.equal(d.adam_m, t.adam_m) and torch.equal(d.adam_v, t.adam_v)
    assert torch.equal(d.flat_grad, t.flat_grad)
    # the 16-bit weight shadows were re-packed once, at the end: the next training forward is that of a fresh model with these weights
    f = Denoiser.from_state_dict(d.state_dict())
    f.train()
    for dat in (data[0], data[n - 1]):              # (both shapes of a mixed group)
        o1, o2 = d.run_pipeline(dat), f.run_pipeline(dat)
        assert torch.equal(o1[PipelineOutput.LOSS], o2[PipelineOutput.LOSS])
        assert torch.equal(o1[PipelineOutput.IMG_DENOISED], o2[PipelineOutput.IMG_DENOISED])
    # a step without accumulate_step calls in front of it is the step of always
    a, b = seeded_denoiser("ssdn", "gauss25", mode, 3), seeded_denoiser("ssdn", "gauss25", mode, 3)
    a.train_step(data[0], lr)
    g = _planned(b, data[0])
    b.adam_steps += 1
    b._last_train_engine.adam(lr, 1, gscale=1.0)
    torch.cuda.synchronize()
    assert torch.equal(a.flat, b.flat) and torch.equal(a.flat_grad, g)


# ---- 8. data parallel ------------------------------------------------------------------------------------------------------------------------
def _group_steps(d, noisy, clean, exchange, halves, nsteps=2, seen=None):
    """nsteps optimiser steps, each over the micro-batches `halves` (row ranges): accumulate_step for all but the last -> (weights, number
    of collectives seen after each call)"""
    from ssdn.datasets import NoisyDataset
    MD = NoisyDataset.Metadata
    counts = []
    d.train()
    for _ in range(nsteps):
        for j, (lo, hi) in enumerate(halves):
            dat = [noisy[lo:hi], None, {MD.INPUT_NOISE_VALUES: torch.full((hi - lo, 1, 1, 1), 25 / 255.0), MD.CLEAN: clean[lo:hi]}]
            if j + 1 < len(halves):
                d.accumulate_step(dat)
            else:
                d.train_step(dat, 3e-4, exchange)
            counts.append(len(seen) if seen is not None else 0)
    torch.cuda.synchronize()
    return d.flat.detach().cpu().numpy().copy(), counts


def _counting(dist, seen):
    orig = dist.all_reduce

    def counting(t, *a, **kw):
        seen.append(t.numel())
        return orig(t, *a, **kw)
    dist.all_reduce = counting
    return orig


def _rccl_world1_accum(port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    import torch.distributed as dist
    from ssdn.hip import dp
    try:
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        clean, noisy = _inputs(4, 64)
        clean, noisy = clean.cuda(), noisy.cuda()
        halves = [(0, 2), (2, 4)]
        plain, _ = _group_steps(_make(), noisy, clean, None, halves)
        d = _make()
        ex = dp.GradExchange(1, d.gradient_exchange(1).ranges, d.device, force_events=True)
        seen = []
        orig = _counting(dist, seen)
        try:
            got, counts = _group_steps(d, noisy, clean, ex, halves, seen=seen)
        finally:
            dist.all_reduce = orig
        nunits = len(ex._units())
        dist.destroy_process_group()
        q.put(("ok", plain, got, counts, nunits))
    except Exception:      # noqa: BLE001
        import traceback
        q.put(("err", traceback.format_exc(), None, None, None))


def test_rccl_world_one_exchanges_once_per_group():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_world1_accum, args=(_free_port(), q))
    p.start()
    tag, plain, got, counts, nunits = q.get(timeout=600)
    p.join(timeout=120)
    assert tag == "ok", plain
    assert np.array_equal(plain, got)               # an identity reduction: the weights of the run without an exchange, bit for bit
    # none in the non-final pass, exactly one set of collectives per optimiser step
    assert nunits >= 2 and counts == [0, nunits, nunits, 2 * nunits], (counts, nunits)


def _gloo_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import torch.distributed as dist
    from ssdn.hip import dp
    r, w, _ = dp.init_from_env("gloo")
    d = _make()
    clean, noisy = _inputs(8, 32)
    ex = d.gradient_exchange(w)
    assert ex.overlapped
    # two global micro-batches of 4 rows; rank r takes its rows of each
    halves = []
    for g in range(2):
        lo, hi = dp.shard_rows(4, r, w)
        halves.append((4 * g + lo, 4 * g + hi))
    seen = []
    orig = _counting(dist, seen)
    try:
        flat, counts = _group_steps(d, noisy, clean, ex, halves, seen=seen)
    finally:
        dist.all_reduce = orig
    q.put((rank, flat, counts, len(ex._units())))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_accumulate_identically():
    import queue
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = {}
    try:
        for _ in range(2):
            r, flat, counts, nunits = q.get(timeout=300)
            got[r] = (flat, counts, nunits)
    except queue.Empty:          # pragma: no cover
        pass
    for p in procs:
        p.join(timeout=120)
        if p.is_alive():
            p.kill()
    assert sorted(got) == [0, 1] and all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert np.array_equal(got[0][0], got[1][0]), "the ranks diverged"
    for r in range(2):
        _, counts, nunits = got[r]
        assert nunits >= 2 and counts == [0, nunits, nunits, 2 * nunits], (counts, nunits)


# ---- 9. against the whole batch ----------------------------------------------------------------------------------------------------------------
def test_two_accumulated_halves_equal_the_whole_batch_step():
    """The whole batch in one step against two half batches accumulated: the same per-sample terms in a different fp32 association -- the
    arithmetic of tests/test_hip_dp.py::test_two_rank_train_step_equals_single_process (two shard sums added by the all-reduce), with that
    test's model, inputs (batch 4 at 32 x 32, split 2 + 2), learning rate, number of steps and bounds."""
    clean, noisy = _inputs(4, 32)
    d = _make()
    want = _steps(d, noisy, clean, None)
    got, _ = _group_steps(_make(), noisy, clean, None, [(0, 2), (2, 4)])
    n = d._n_main
    p0 = _make().flat.detach().cpu().numpy()[:n]
    upd_w, upd_g = want[:n] - p0, got[:n] - p0
    cos = float((upd_w * upd_g).sum() / (np.linalg.norm(upd_w) * np.linalg.norm(upd_g) + 1e-30))
    frac_off = float(np.mean(np.abs(upd_w - upd_g) > 0.5 * 3e-4))
    # the raw gradients at the initial weights: mean over the whole batch against the mean of the two half-batch means
    from ssdn.datasets import NoisyDataset
    MD = NoisyDataset.Metadata
    t = _make()
    t.train()

    def grad(lo, hi):
        t.run_pipeline([noisy[lo:hi], None, {MD.INPUT_NOISE_VALUES: torch.full((hi - lo, 1, 1, 1), 25 / 255.0), MD.CLEAN: clean[lo:hi]}])
        t.backward()
        return t.flat_grad[:n].double().cpu()
    g_whole, g_halves = grad(0, 4), 0.5 * (grad(0, 2) + grad(2, 4))
    cos_g = float((g_whole @ g_halves) / (g_whole.norm() * g_halves.norm()))
    print("whole batch vs two accumulated halves: cosine of the updates %.6f, share of weights off by > lr/2 %.5f, cosine of the raw "
          "gradients %.8f" % (cos, frac_off, cos_g))
    assert cos >= 0.999, cos
    assert frac_off <= 0.01, frac_off


# ---- 10. the CLI -----------------------------------------------------------------------------------------------------------------------------
def test_cli_train_with_accumulate_and_resume(tmp_path):
    from ssdn.__main__ import start_cli
    from ssdn.datasets import h5lite
    from ssdn.params import StateValue
    from test_hip_trainer import _scalars
    rng = np.random.RandomState(3)
    yy, xx = np.mgrid[0:48, 0:56]
    imgs = []
    for i in range(12):
        base = 0.5 + 0.35 * np.sin(xx / (5.0 + i) + i) * np.cos(yy / (7.0 + i))
        img = np.stack([base, np.roll(base, 3 * i, 1), 1 - base], 0) + rng.rand(3, 48, 56) * 0.05
        imgs.append(np.uint8(np.clip(img, 0, 1) * 255))
    path = str(tmp_path / "small_train.h5")
    h5lite.write_dataset_file(path, imgs)
    runs = str(tmp_path / "runs")
    torch.manual_seed(20261016)
    # 20 optimiser steps of 2 minibatches of 4
    tr = start_cli(["train", "start", "-a", "ssdn", "-n", "gauss25", "--noise_value", "known", "-t", path, "-i", "160",
                    "--train_batch_size", "4", "--patch_size", "32", "--print_interval", "40", "--checkpoint_interval", "80",
                    "--accumulate", "2", "--runs_dir", runs])
    run = tr.run_dir_path
    assert tr.accumulate == 2 and tr.state[StateValue.ITERATION] == 160 and tr.denoiser.adam_steps == 20
    log = open(os.path.join(run, "log.txt")).read()
    assert "Gradient accumulation: 2 minibatches" in log and "TRAINING FINISHED" in log
    tfiles = sorted(os.path.basename(p) for p in glob.glob(os.path.join(run, "training", "*.training")))
    assert tfiles == ["model_00000000.training", "model_00000080.training", "model_00000160.training"]
    sd = torch.load(os.path.join(run, "training", "model_00000160.training"), weights_only=False)
    assert sd["accumulate"] == 2 and float(sd["optimizer"]["state"][0]["step"]) == 20.0
    sc = _scalars(run)
    assert [s for s, _ in sc["train/loss"]] == [40, 80, 120, 160] and all(np.isfinite(v) for _, v in sc["train/loss"])
    # resume: K comes back from the file; 32 more images = 4 more optimiser steps
    t2 = start_cli(["train", "resume", run, "-i", "192"])
    assert t2.accumulate == 2 and t2.state[StateValue.ITERATION] == 192 and t2.denoiser.adam_steps == 24
    sd = torch.load(os.path.join(run, "training", "model_00000192.training"), weights_only=False)
    assert sd["accumulate"] == 2 and float(sd["optimizer"]["state"][0]["step"]) == 24.0
    assert all(np.isfinite(v) for _, v in _scalars(run)["train/loss"])
    assert torch.isfinite(t2.denoiser.flat).all()
    # ... and the flag overrides the stored value
    t3 = start_cli(["train", "resume", run, "-i", "200", "--accumulate", "1"])
    assert t3.accumulate == 1 and t3.denoiser.adam_steps == 26
    assert "accumulate" not in torch.load(os.path.join(run, "training", "model_00000200.training"), weights_only=False)
