"""CPU: the execution order and lanes of the backward list are part of the plan (ssdn/hip/graph.py::NetPlan.bwd_sched).
* tests/golden/g_bwd_sched.json (oracle/gen_bwd_sched.py) pins the schedule of 112 plans: generated from the engine's ordering code the
  commit before the scheduler moved into the planner, so "the planner emits what the engine emitted" is a file comparison;
* the engine materialises exactly that list, whatever the planner constants are by then (a plan is self-contained);
* the interpreter computes bit-identical gradients in the data-flow order (plan.bwd) and in the scheduled one."""
import copy
import json
import os

import pytest
import torch

import gen_bwd_sched as GEN
import restate as R
from interp import Interp
from ssdn.hip import graph as G
from ssdn.hip import lib as L
from ssdn.hip.engine import DeviceNet
from test_lowering_cpu import flat_params

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GEN.NAME)) as _f:
    GOLD = {(c["wgrad_mega"], c["input_grad"], c["cus"], tuple(c["shape"])): c for c in json.load(_f)}
BASE, TINY = (3, 9, True, 32, 64, 64), (1, 2, True, 2, 32, 32)


def test_fixture_holds_the_full_product():
    assert len(GOLD) == len(GEN.CASES) == 112 and set(GOLD) == set(GEN.CASES)


@pytest.mark.parametrize("mode,ig,cus,shape", GEN.CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_schedule_is_the_fixtures(mode, ig, cus, shape):
    saved = G.WGRAD_MEGA
    plan = GEN.make_plan(mode, ig, cus, shape)
    assert G.WGRAD_MEGA == saved
    assert sorted(i for i, _ in plan.bwd_sched) == list(range(len(plan.bwd))), "a permutation of plan.bwd"
    assert GEN.case_record(mode, ig, cus, shape, plan, plan.bwd_sched) == GOLD[(mode, ig, cus, shape)]


def test_inference_plan_has_no_schedule():
    plan = G.NetPlan("m/", 3, 9, True, 2, 32, 32, cus=256, train=False)
    assert plan.bwd == [] and plan.bwd_sched == []


def _materialised(plan):
    flat = torch.zeros(plan.nparams)
    dn = DeviceNet(plan, torch.device("cpu"), flat, torch.zeros_like(flat))
    return [(int(dn.bwd.arr[i].type), int(dn.bwd.arr[i].lane)) for i in range(dn.bwd.n)]


def _expected(plan, gold):
    assert len(plan.bwd) == gold["n"] and GEN.digest(plan) == gold["ops"]
    return [(L.OP[plan.bwd[i].type], lane) for i, lane in gold["sched"]]


@pytest.mark.parametrize("mode,shape", [("split", BASE), (None, BASE), ("split", TINY)])
def test_engine_materialises_the_schedule(mode, shape):
    plan = GEN.make_plan(mode, False, 256, shape)
    assert _materialised(plan) == _expected(plan, GOLD[(mode, False, 256, shape)])


def test_plan_is_self_contained():
    """the launch groups and lanes are fixed when the plan is built: materialising it under another WGRAD_MEGA changes nothing"""
    plan = GEN.make_plan("split", False, 256, BASE)
    saved = G.WGRAD_MEGA
    G.WGRAD_MEGA = "all"
    try:
        got = _materialised(plan)
    finally:
        G.WGRAD_MEGA = saved
    assert got == _expected(plan, GOLD[("split", False, 256, BASE)])
    assert got != _expected(plan, GOLD[("all", False, 256, BASE)])


@pytest.mark.parametrize("shape,mega", [((3, 9, True, 2, 64, 64), True), (TINY, False)])
def test_interpreter_runs_the_scheduled_order(shape, mega):
    """Every op is a pure function of its inputs: a legal order gives the data-flow order's gradients bit for bit, an op moved in front of
    its producer does not.  32768 full-resolution pixels (8 rotated images of 64x64) is the smallest plan on the chip-wide path."""
    cin, cout, bs, B, H, W = shape
    plan = G.NetPlan("m/", cin, cout, bs, B, H, W, cus=256)
    assert bool(plan._mega_ops) == mega
    it = Interp(plan, flat_params(plan, R.make_params(cin, cout, bs, seed=7)), fp16=False)
    it.t["m/in32"] = R.hash_tensor((B, cin, H, W), 91, 0, 1)
    it.t["m/g32"] = R.hash_tensor((B, cout, H, W), 92, -1, 1) * 1e-3
    it.run(plan.pack)
    it.run(plan.fwd)
    it2 = copy.deepcopy(it)
    it.run(plan.bwd)
    it2.run([plan.bwd[i] for i, _ in plan.bwd_sched])
    assert float(it.grads.abs().max()) > 0 and torch.equal(it.grads, it2.grads)
    # every gradient tensor (bf16 on the device) the list writes -- and everything else the interpreter holds
    assert set(it.t) == set(it2.t) and sum(1 for name in it.t if name in plan.tensors and plan.tensors[name].kind == "actb") >= 25
    for name in it.t:
        assert torch.equal(it.t[name], it2.t[name]), name
