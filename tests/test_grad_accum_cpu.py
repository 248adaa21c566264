"""CPU side of gradient accumulation over micro-batches: the ABI mirror of the accumulating slab reduction,
the in-place toggle on a `DeviceNet` built on CPU tensors, the trainer's grouping of minibatches into optimiser steps (with a stub in
the place of the HIP step, single process and two gloo ranks) and the `--accumulate` flag of `ssdn train`."""
import ctypes as C
import glob
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import ssdn
from ssdn.datasets import NoisyDataset, h5lite
from ssdn.hip import lib as L
from ssdn.params import ConfigValue, NoiseAlgorithm, NoiseValue, PipelineOutput, StateValue


# ---- 1. ABI mirror and the toggle --------------------------------------------------------------------------------------------------
def test_wreduce_args_end_in_accumulate_and_abi_is_19():
    assert L.WreduceArgs._fields_[-1] == ("accumulate", C.c_int32)
    assert L.ABI_VERSION == 19
    assert L.OP["accum"] == 25 and L.ARG_TYPES["accum"] is L.AccumArgs
    assert C.sizeof(L.WreduceArgs) == 88          # 32 entries of the merged launch's table stay under the 4 KB kernel-argument limit
    assert 32 * C.sizeof(L.WreduceArgs) + 4 * (33 + 32 + 32 + 1) < 4096


def _nets():
    from ssdn.hip.engine import DeviceNet
    from ssdn.hip.graph import NetPlan
    for plan in (NetPlan("m/", 3, 9, True, 32, 64, 64, cus=256), NetPlan("s/", 3, 1, False, 32, 64, 64, cus=256)):
        flat = torch.zeros(plan.nparams)
        yield DeviceNet(plan, torch.device("cpu"), flat, torch.zeros_like(flat))


def _lists(dn):
    """every variant of the backward list a DeviceNet hands out: (type code, argument struct) of each record"""
    from ssdn.hip import dp
    out = [[(int(dn.bwd.arr[i].type), dn.bwd.args[i]) for i in range(dn.bwd.n)]]
    if dn.bwd_head is not None:
        out.append([(int(dn.bwd_head.arr[i].type), dn.bwd_head.args[i]) for i in range(dn.bwd_head.n)])
    out.append([(L.OP[ty], a) for ty, a in dn.tail_recs])
    ev = dn.bwd_with_events(dp.bucket_layers(dn.plan.layers), lambda ks: 1000 + sum(ks))
    out.append([(int(ev.arr[i].type), ev.args[i]) for i in range(ev.n)])
    return out


def test_set_accumulate_flips_only_the_flag_of_every_reduction_in_every_list_variant():
    off, width = L.WreduceArgs.accumulate.offset, L.WreduceArgs.accumulate.size
    for dn in _nets():
        lists = _lists(dn)
        before = [[bytes(a) for _, a in lst] for lst in lists]
        nred = [sum(1 for ty, _ in lst if ty == L.OP["wreduce"]) for lst in lists]
        assert nred[0] > 10 and nred[-1] == nred[0]                      # bwd and the event-carrying list hold every reduction
        if dn.bwd_head is not None:
            assert nred[1] + nred[2] == nred[0] and nred[2] > 0          # head + deferred tail
        for lst in lists:
            assert all(a.accumulate == 0 for ty, a in lst if ty == L.OP["wreduce"])
        dn.set_accumulate(True)
        dn.set_accumulate(True)                                          # idempotent
        for lst, raw in zip(lists, before):
            for (ty, a), b in zip(lst, raw):
                now = bytes(a)
                if ty == L.OP["wreduce"]:
                    assert a.accumulate == 1
                    assert now[:off] == b[:off] and now[off + width:] == b[off + width:]
                else:
                    assert now == b
        # a list built while the flag is on shares the same structs too
        assert all(a.accumulate == 1 for ty, a in _lists(dn)[-1] if ty == L.OP["wreduce"])
        dn.set_accumulate(False)
        for lst, raw in zip(lists, before):
            assert [bytes(a) for _, a in lst] == raw


# ---- 2. trainer grouping ---------------------------------------------------------------------------------------------------------------
B, P, NIMG, K = 4, 32, 23, 3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _images():
    rng = np.random.RandomState(7)
    imgs = []
    for i in range(NIMG):
        im = rng.randint(0, 256, size=(3, 40 + i % 5, 37 + i % 3), dtype=np.uint8)
        im[0] = i
        imgs.append(im)
    return imgs


def _cfg(path, batch, iters, snapshot=10 ** 9):
    cfg = ssdn.cfg.base()
    cfg[ConfigValue.ALGORITHM] = NoiseAlgorithm.SELFSUPERVISED_DENOISING
    cfg[ConfigValue.NOISE_STYLE] = "gauss25"
    cfg[ConfigValue.NOISE_VALUE] = NoiseValue.KNOWN
    cfg[ConfigValue.TRAIN_ITERATIONS] = iters
    cfg[ConfigValue.TRAIN_MINIBATCH_SIZE] = batch
    cfg[ConfigValue.TRAIN_PATCH_SIZE] = P
    cfg[ConfigValue.TRAIN_DATA_PATH] = path
    cfg[ConfigValue.DATALOADER_WORKERS] = 0
    cfg[ConfigValue.PRINT_INTERVAL] = 4
    cfg[ConfigValue.EVAL_INTERVAL] = 10 ** 9
    cfg[ConfigValue.SNAPSHOT_INTERVAL] = snapshot
    return cfg


def _g(idx, n):
    return torch.sin(torch.arange(n, dtype=torch.float64) * 0.013 * (idx + 1)).to(torch.float32)


def _make_stub(cfg):
    from ssdn.denoiser import Denoiser
    from ssdn.hip import dp

    class StubDenoiser(Denoiser):
        """fake gradients that depend only on WHICH images a minibatch holds; accumulate_step adds one to the running sum, train_step adds
        its own, exchanges through the driver the HIP step uses and applies the mean over the group"""

        def __init__(self, cfg):
            super().__init__(cfg, device="cpu")
            self.calls, self.lrs, self.nterms = [], [], 0

        def _grad(self, data, kind):
            idx = [int(i) for i in data[NoisyDataset.METADATA][NoisyDataset.Metadata.INDEXES]]
            self.calls.append((kind, idx))
            g = torch.stack([_g(i, self.flat.numel()) for i in idx]).mean(0)
            if self.nterms == 0:
                self.flat_grad.copy_(g)
            else:
                self.flat_grad.add_(g)
            self.nterms += 1

        def _out(self, data):
            inp, clean = data[NoisyDataset.INPUT], data[NoisyDataset.METADATA][NoisyDataset.Metadata.CLEAN]
            n = inp.shape[0]
            return {PipelineOutput.INPUTS: data, PipelineOutput.LOSS: torch.ones(n, 1), PipelineOutput.IMG_DENOISED: clean.clone(),
                    PipelineOutput.IMG_MU: inp.clone(), PipelineOutput.NOISE_STD_DEV: torch.ones(n, 1, 1), PipelineOutput.MODEL_STD_DEV: torch.ones(n, P, P)}

        def accumulate_step(self, data, metrics=False):
            self._grad(data, "accumulate_step")
            return self._out(data)

        def train_step(self, data, lr, exchange=None):
            self.lrs.append(lr)
            scale = dp.exchange_step(lambda ex: self._grad(data, "train_step"), self.flat_grad, exchange)
            self.flat.sub_(0.5 * scale / self.nterms * self.flat_grad)      # lr-free update: lr(0) = 0 would hide everything
            self.nterms = 0
            return self._out(data)
    return StubDenoiser(cfg)


def _by_hand(order, batch, k, init):
    """the update of the mean over each group's minibatches, each minibatch's gradient the mean over its images"""
    flat = init.clone()
    mbs = [order[i:i + batch] for i in range(0, len(order), batch)]
    for j in range(0, len(mbs), k):
        grp = mbs[j:j + k]
        s = None
        for ids in grp:
            g = torch.stack([_g(i, flat.numel()) for i in ids]).mean(0)
            s = g if s is None else s + g
        flat.sub_(0.5 * 1.0 / len(grp) * s)
    return flat


def _single_run(path, runs, batch, iters, k, snapshot=10 ** 9):
    from ssdn.train import DenoiserTrainer
    torch.manual_seed(5)
    tr = DenoiserTrainer(_cfg(path, batch, iters, snapshot), runs_dir=runs)
    tr.accumulate = k
    tr.denoiser = _make_stub(tr.cfg)
    tr.init_state()
    init = tr.denoiser.flat.clone()
    tr.train()
    return tr, init


def test_trainer_groups_minibatches_into_optimiser_steps(tmp_path):
    from ssdn.train import resume_run
    from ssdn.utils.utils import compute_ramped_lrate
    path = str(tmp_path / "train_set.h5")
    h5lite.write_dataset_file(path, _images())
    iters = 44                                        # 11 minibatches of 4: groups of 3, 3, 3 and a short one of 2
    tr, init = _single_run(path, str(tmp_path / "runs"), B, iters, K, snapshot=4)
    d = tr.denoiser
    kinds = [c[0] for c in d.calls]
    assert kinds == (["accumulate_step"] * 2 + ["train_step"]) * 3 + ["accumulate_step", "train_step"]
    assert all(len(c[1]) == B for c in d.calls)
    assert tr.state[StateValue.ITERATION] == iters
    # the learning rate: read once per group = the K = 1 run with the K-fold minibatch
    want_lr = [compute_ramped_lrate(i, iters, 0.1, 0.3, 3e-4) for i in range(0, iters, K * B)]
    assert d.lrs == pytest.approx(want_lr, rel=0, abs=0)
    tr1, _ = _single_run(path, str(tmp_path / "runs1"), K * B, iters, 1)
    assert tr1.denoiser.lrs == d.lrs
    assert [c[0] for c in tr1.denoiser.calls] == ["train_step"] * 4
    # interval checks at group boundaries only: SNAPSHOT_INTERVAL = 4 divides every ITERATION a minibatch ends on, files exist for the
    # boundaries 0, 12, 24, 36 and the end
    snaps = sorted(int(os.path.basename(p)[6:14]) for p in glob.glob(os.path.join(tr.run_dir_path, "training", "*.training")))
    assert snaps == [0, 12, 24, 36, 44]
    # the parameters: the by-hand update over the order the run consumed
    order = [i for c in d.calls for i in c[1]]
    assert len(order) == iters
    assert torch.allclose(d.flat, _by_hand(order, B, K, init), rtol=0, atol=2e-6)
    # `.training`: the extra key when K > 1, the key set of always when K = 1; resume restores K
    sd = torch.load(os.path.join(tr.run_dir_path, "training", "model_%08d.training" % iters), map_location="cpu", weights_only=False)
    assert sd["accumulate"] == K
    sd1 = torch.load(os.path.join(tr1.run_dir_path, "training", "model_%08d.training" % iters), map_location="cpu", weights_only=False)
    assert "accumulate" not in sd1 and set(sd) - set(sd1) == {"accumulate"}
    assert resume_run(tr.run_dir_path).accumulate == K
    assert resume_run(tr1.run_dir_path).accumulate == 1


GB, ITERS2 = 8, 52            # two ranks: 6 global minibatches of 8 + an un-sharded tail of 4 = groups of 3, 3 and a short one of 1


def _worker(rank, world, port, path, runs, out):
    torch.cuda.is_available = lambda: False
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    torch.manual_seed(100 + rank)
    import torch.distributed as dist
    from ssdn.train import DenoiserTrainer
    tr = DenoiserTrainer(_cfg(path, GB, ITERS2), runs_dir=runs)
    tr.accumulate = K
    tr.denoiser = _make_stub(tr.cfg)
    tr.init_state()
    tr.train()
    d = tr.denoiser
    out.put((rank, d.calls, d.lrs, d.flat.numpy().copy(), tr.state[StateValue.ITERATION], len(tr._shard.counts)))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_trainer_accumulates_like_a_single_process(tmp_path):
    from ssdn.datasets import FixedLengthSampler
    from ssdn.utils.utils import compute_ramped_lrate
    path = str(tmp_path / "train_set.h5")
    h5lite.write_dataset_file(path, _images())
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, path, str(tmp_path / "runs"), out)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(world):
        r = out.get(timeout=300)
        res[r[0]] = r[1:]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    torch.manual_seed(1234)
    order = list(FixedLengthSampler(list(range(NIMG)), num_samples=ITERS2, shuffled=True).sampler())
    kinds = (["accumulate_step"] * 2 + ["train_step"]) * 2 + ["train_step"]
    per = GB // world
    for rank in range(world):
        calls, lrs, _, it, left = res[rank]
        assert [c[0] for c in calls] == kinds
        for k in range(6):
            assert calls[k][1] == order[k * GB + rank * per: k * GB + (rank + 1) * per]
        assert calls[6][1] == order[6 * GB:]                              # the tail: un-sharded, a group of its own
        assert it == ITERS2 and left == 0
        assert lrs == [compute_ramped_lrate(i, ITERS2, 0.1, 0.3, 3e-4) for i in (0, K * GB, 2 * K * GB)]
    assert np.array_equal(res[0][2], res[1][2])                            # replicas identical
    torch.manual_seed(100)                                                 # ... and equal to one process over the same order from rank 0's init
    rcfg = _cfg(path, GB, ITERS2)
    ssdn.cfg.infer(rcfg)
    ref = _make_stub(rcfg)
    assert np.allclose(res[0][2], _by_hand(order, GB, K, ref.flat).numpy(), rtol=0, atol=2e-6)


# ---- 3. CLI ----------------------------------------------------------------------------------------------------------------------------
def _parser():
    import argparse
    from ssdn.cli.cmds.train import TrainCommand
    parser = argparse.ArgumentParser()
    TrainCommand().configure(parser.add_subparsers(dest="cmd"))
    return parser


def test_cli_accumulate_flag_parses_and_rejects_less_than_one(capsys):
    p = _parser()
    start = ["train", "start", "-t", "x.h5", "-i", "100", "-a", "ssdn", "-n", "gauss25", "--noise_value", "known"]
    assert p.parse_args(start).accumulate is None
    assert p.parse_args(start + ["--accumulate", "4"]).accumulate == 4
    assert p.parse_args(["train", "resume", "some/run", "--accumulate", "2"]).accumulate == 2
    assert p.parse_args(["train", "resume", "some/run"]).accumulate is None
    for bad in ("0", "-3", "two"):
        with pytest.raises(SystemExit):
            p.parse_args(start + ["--accumulate", bad])
        with pytest.raises(SystemExit):
            p.parse_args(["train", "resume", "some/run", "--accumulate", bad])
    capsys.readouterr()
