#!/usr/bin/env python3
"""TEST INFRASTRUCTURE -- writes tests/golden/g_bwd_sched.json: the execution order and lanes of the backward list
(ssdn.hip.graph.NetPlan.bwd_sched) of a grid of plans -- every weight-gradient mode x with / without the input gradient x a big and a
small device x seven network shapes.  tests/test_bwd_sched_cpu.py compares the planner with this file, so a change of the schedule shows
up as this file's diff: regenerate it ON PURPOSE only.

    python oracle/gen_bwd_sched.py            # pure Python: neither the library nor a device is needed

One case per line: the plan's arguments, len(plan.bwd), a digest of the (type, layer) of every op of plan.bwd (an index of the schedule
provably names the same op) and the [index into plan.bwd, lane] pairs in execution order.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "selfsupervised-denoising_amd"))

from ssdn.hip import graph as G  # noqa: E402

OUT = os.environ.get("SSDN_GOLDEN_OUT") or os.path.join(os.path.dirname(HERE), "tests", "golden")
NAME = "g_bwd_sched.json"
MODES = ("split", "all", "buckets", None)
SHAPES = [(3, 9, True, 32, 64, 64), (3, 3, False, 4, 64, 64), (1, 2, True, 2, 32, 32), (3, 9, True, 16, 128, 128),
          (3, 1, False, 32, 64, 64), (3, 3, False, 4, 64, 96), (1, 1, False, 32, 64, 64)]      # (cin, cout, blindspot, B, H, W)
CASES = [(mode, ig, cus, shape) for mode in MODES for ig in (False, True) for cus in (256, 32) for shape in SHAPES]


def make_plan(mode, input_grad, cus, shape):
    """the plan of one case, built under graph.WGRAD_MEGA = mode (restored afterwards)"""
    cin, cout, bs, B, H, W = shape
    saved = G.WGRAD_MEGA
    G.WGRAD_MEGA = mode
    try:
        return G.NetPlan("m/", cin, cout, bs, B, H, W, cus=cus, input_grad=input_grad)
    finally:
        G.WGRAD_MEGA = saved


def digest(plan) -> str:
    return hashlib.sha256(json.dumps([[op.type, op.a.get("layer")] for op in plan.bwd]).encode()).hexdigest()[:16]


def case_record(mode, input_grad, cus, shape, plan, sched) -> dict:
    return dict(wgrad_mega=mode, input_grad=input_grad, cus=cus, shape=list(shape), n=len(plan.bwd), ops=digest(plan),
                sched=[[int(i), int(lane)] for i, lane in sched])


def generate(schedule=lambda plan, mode: plan.bwd_sched) -> str:
    """the file's text.  schedule(plan, mode) -> [(index into plan.bwd, lane)] in execution order"""
    lines = []
    for mode, ig, cus, shape in CASES:
        plan = make_plan(mode, ig, cus, shape)
        lines.append(json.dumps(case_record(mode, ig, cus, shape, plan, schedule(plan, mode)), separators=(",", ":")))
    return "[\n" + ",\n".join(lines) + "\n]\n"


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    text = generate()
    with open(os.path.join(OUT, NAME), "w") as f:
        f.write(text)
    print("wrote %s: %d cases, %d bytes, sha256 %s" % (os.path.join(OUT, NAME), len(CASES), len(text), hashlib.sha256(text.encode()).hexdigest()))
