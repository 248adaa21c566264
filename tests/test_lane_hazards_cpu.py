"""CPU: the planner's half of the lane contract (include/ssdn_hip.h, the comment on `ssdn_op`): "The planner guarantees the absence of
WAR/WAW hazards between lanes".  tests/lane_model.py holds the contract as a model -- a happens-before relation over (op, lane) lists and a
table of what every planner op reads and writes, channel range by channel range.  Here:
  * the table is honest: the interpreter (oracle/interp.py), run with its recording hook, touches exactly the regions the table names;
  * no plan races: hazards() is empty for the schedule of every plan of the schedule fixture and of the non-square shapes, for every
    backward list the engine materialises from a plan (whole, with the deferred tail, with event marks and the buckets' collectives) --
    and every region a side-lane op reads has all of its writers ordered before that read;
  * the checker has teeth: four broken schedules of BASELINE config 2 are each reported, with the class of the hazard."""
import copy

import pytest
import torch

import gen_bwd_sched as GEN
import lane_model as LM
import restate as R
from interp import Interp
from ssdn.hip import graph as G
from ssdn.hip import lib as L
from ssdn.hip.dp import bucket_layers, bucket_ranges
from ssdn.hip.engine import DeviceNet
from ssdn.hip.graph import NetPlan, View
from test_hip_ops import HW_CASES
from test_lowering_cpu import flat_params

BASE = (3, 9, True, 32, 64, 64)             # BASELINE config 2


# ---- the table is honest -----------------------------------------------------------------------------------------------------------------
def _table_as_the_interpreter_sees_it(plan, op):
    """lane_model.accesses(op), less the two places where the device reads a derived copy the interpreter does not model:
    the chunk-major weight copies (wfc/ wdc/: a layout of the library, oracle/interp.py::op_wpack) and the route words of a stand-alone
    SSDN_OP_POOL_BWD (the interpreter always reads the activation the words were derived from)."""
    acc = {r for r in LM.accesses(plan, op) if not r[0].startswith((plan.prefix + "wfc/", plan.prefix + "wdc/"))}
    if op.type == "pool_bwd" and op.a.get("route") is not None:
        acc.discard((op.a["route"], 0, LM.WHOLE, "r"))
        acc.add((op.a["act"].t, op.a["act"].co, op.a["act"].co + op.a["C"], "r"))
    return acc


@pytest.mark.parametrize("shape", [(1, 2, True, 2, 32, 32), (3, 9, True, 2, 32, 32), (3, 3, False, 2, 32, 64), (3, 9, True, 4, 64, 64)],
                         ids=lambda s: "x".join(map(str, s)))
def test_table_equals_what_the_interpreter_touches(shape):
    cin, cout, bs, B, H, W = shape
    plan = NetPlan("m/", cin, cout, bs, B, H, W, cus=256)
    it = Interp(plan, flat_params(plan, R.make_params(cin, cout, bs, seed=7)), fp16=False, record=True)
    it.t["m/in32"] = R.hash_tensor((B, cin, H, W), 91, 0, 1)
    it.t["m/g32"] = R.hash_tensor((B, cout, H, W), 92, -1, 1) * 1e-3
    ops = plan.pack + plan.fwd + plan.bwd
    it.run(ops)
    assert len(it.rec) == len(ops)
    seen = set()
    for k, (op, got) in enumerate(zip(ops, it.rec)):
        want = _table_as_the_interpreter_sees_it(plan, op)
        assert got == want, "op %d %s %s: only recorded %s, only in the table %s" % \
            (k, op.type, op.a.get("layer", ""), sorted(got - want), sorted(want - got))
        seen.add(op.type)
        seen.update(key for key in ("urot", "unrot_smask", "upsum", "mask_sign", "upsum_mask_sign", "sign_out", "pool", "route")
                    if op.a.get(key) is not None)
        for name, lo, hi, _ in LM.accesses(plan, op):            # every region lies inside its tensor
            spec = plan.tensors.get(name)
            if spec is not None and spec.kind in ("act", "actb"):
                assert 0 <= lo < hi <= spec.shape[-1], (op.type, name, lo, hi)
            elif name in ("params", "grads"):
                assert plan.param_base <= lo < hi <= plan.param_base + plan.nparams
    if shape == (3, 9, True, 4, 64, 64):      # the smallest plan with the fused UNROT_FWD, sign bytes and the fused UPSUM_BWD
        # (upsum_mask_sign needs 256 tiles at 32x32, batch 8: the one argument of the table no plan here exercises)
        assert {"urot", "unrot_smask", "upsum", "mask_sign", "sign_out"} <= seen, seen
    assert {"pack_input", "wpack", "conv", "grad_pack", "wgrad", "wreduce", "pool_bwd"} <= seen


def test_recording_only_observes():
    """a recording run and a plain one leave the same bits"""
    cin, cout, bs, B, H, W = 1, 2, True, 2, 32, 32
    plan = NetPlan("m/", cin, cout, bs, B, H, W, cus=256)
    runs = []
    for record in (False, True):
        it = Interp(plan, flat_params(plan, R.make_params(cin, cout, bs, seed=7)), fp16=True, record=record)
        it.t["m/in32"] = R.hash_tensor((B, cin, H, W), 91, 0, 1)
        it.t["m/g32"] = R.hash_tensor((B, cout, H, W), 92, -1, 1) * 1e-3
        it.run(plan.pack + plan.fwd + plan.bwd)
        runs.append(it)
    a, b = runs
    assert a.rec is None and len(b.rec) == len(plan.pack + plan.fwd + plan.bwd)
    assert torch.equal(a.grads, b.grads) and set(a.t) == set(b.t)
    for name in a.t:
        assert torch.equal(a.t[name], b.t[name]), name


# ---- the model itself --------------------------------------------------------------------------------------------------------------------
def test_happens_before_is_the_headers():
    """lanes 1 and 3 after lane 0 and themselves; lane 2 after 0, 1, 3 and itself; nothing else; the join after everything; a mark stands
    for its own lane's prefix"""
    items = [LM.Item("op", l) for l in (0, 1, 3, 2, 0, 1, 3, 2)] + [LM.Item("mark", 1), LM.Item("join")]
    pred = LM.happens_before(items)
    before = lambda j: {i for i in range(len(items)) if (pred[j] >> i) & 1}      # noqa: E731
    assert before(0) == set() and before(1) == {0} and before(2) == {0} and before(3) == {0, 1, 2}
    assert before(4) == {0}, "the main lane never waits for a side lane inside a list"
    assert before(5) == {0, 1, 4} and before(6) == {0, 2, 4} and before(7) == {0, 1, 2, 3, 4, 5, 6}
    assert before(8) == {0, 1, 4, 5}, "a mark on lane 1: lane 1's prefix and the lane-0 ops that prefix waited for"
    assert before(9) == set(range(9))
    ext = items[:9] + [LM.Item("ext", waits=[8])]
    assert {i for i in range(10) if (LM.happens_before(ext)[9] >> i) & 1} == {0, 1, 4, 5, 8}


# ---- no plan races -----------------------------------------------------------------------------------------------------------------------
def _clean(plan, sched, what):
    found = LM.hazards(plan, sched)
    assert not found, "%s:\n%s" % (what, LM.describe(plan, sched, found))
    # the premise the header leans on: what a side lane reads has no writer that is not ordered before the read
    loose = LM.unordered_writers(plan, sched)
    assert not loose, "%s: side-lane reads with an unordered writer: %s" % (what, loose[:5])


@pytest.mark.parametrize("mode,ig,cus,shape", GEN.CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_no_schedule_of_the_fixture_races(mode, ig, cus, shape):
    plan = GEN.make_plan(mode, ig, cus, shape)
    assert sorted(i for i, _ in plan.bwd_sched) == list(range(len(plan.bwd)))
    _clean(plan, plan.bwd_sched, "bwd_sched")


@pytest.mark.parametrize("case", sorted({c[:7] for c, _ in HW_CASES}), ids=lambda c: "x".join(map(str, c)))
def test_no_schedule_of_the_non_square_shapes_races(case):
    cin, cout, bs, B, H, W, cus = case
    for mode in GEN.MODES:
        plan = GEN.make_plan(mode, False, cus or 256, (cin, cout, bs, B, H, W))
        _clean(plan, plan.bwd_sched, "bwd_sched under WGRAD_MEGA = %s" % mode)


def _device_net(mode, shape):
    plan = GEN.make_plan(mode, False, 256, shape)
    flat = torch.zeros(plan.nparams)
    return plan, DeviceNet(plan, torch.device("cpu"), flat, torch.zeros_like(flat))


def _is_list(ol, plan, sched):
    """the materialised list `ol` is `sched` (marks included), record by record"""
    want = [(L.OP["event_record"], e[1]) if e[0] == "mark" else (L.OP[plan.bwd[e[0]].type], e[1]) for e in sched]
    assert [(int(ol.arr[i].type), int(ol.arr[i].lane)) for i in range(ol.n)] == want


def _events_sched(plan, dn, drop=None):
    """bwd_with_events as a sched: the list with its marks, then every gradient bucket's collective -- a reader of the bucket's range of the
    flat gradient that waits for exactly the bucket's marks.  drop = (bucket, lane): the bucket's collective does not wait for its mark on
    that lane.  -> (sched, OpList, marks)"""
    buckets = bucket_layers(plan.layers)
    ol = dn.bwd_with_events(buckets, lambda ks: 7000 + sum(1 << k for k in ks))
    mark_at = {pos: (lane, ks) for pos, lane, ks in ol.marks}
    sched, waits, rest = [], {}, iter(plan.bwd_sched)
    for pos in range(ol.n):
        if pos in mark_at:
            lane, ks = mark_at[pos]
            for k in ks:
                if drop != (k, lane):
                    waits.setdefault(k, []).append(len(sched))
            sched.append(("mark", lane))
        else:
            sched.append(next(rest))
    assert next(rest, None) is None
    _is_list(ol, plan, sched)
    ranges = bucket_ranges(plan.layers, plan.nparams, plan.nparams)
    for k, (lo, hi) in enumerate(ranges):
        if hi > lo:
            sched.append(("ext", [("grads", plan.param_base + lo, plan.param_base + hi, "r")], waits.get(k, [])))
    return sched + [("join",)], ol, mark_at


@pytest.mark.parametrize("mode,shape", [(m, BASE) for m in GEN.MODES] + [("split", (3, 3, False, 4, 64, 64)), ("split", (1, 2, True, 2, 32, 32)),
                                                                         ("split", (3, 9, True, 16, 128, 128))],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_no_materialised_backward_list_races(mode, shape):
    plan, dn = _device_net(mode, shape)
    # the whole list
    sched = list(plan.bwd_sched)
    _is_list(dn.bwd, plan, sched)
    _clean(plan, sched + [("join",)], "bwd")
    # the deferred tail: the list without its closing reductions, its join, then those reductions on the caller's stream
    if dn.tail_recs:
        nt = len(dn.tail_recs)
        assert all(plan.bwd[i].type == "wreduce" for i, _ in sched[-nt:])
        _is_list(dn.bwd_head, plan, sched[:-nt])
        _clean(plan, sched[:-nt] + [("join",)] + [(i, 0) for i, _ in sched[-nt:]] + [("join",)], "bwd_head | tail")
    # with event marks: every bucket's collective reads its range behind exactly the marks it waits for
    ev, ol, mark_at = _events_sched(plan, dn)
    assert len(mark_at) >= 1 and sum(1 for e in ev if e[0] == "ext") == 4
    _clean(plan, ev, "bwd_with_events")


# ---- the checker has teeth ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base():
    plan, dn = _device_net("split", BASE)
    acc = [LM.accesses(plan, plan.bwd[i]) for i, _ in plan.bwd_sched]
    return plan, dn, list(plan.bwd_sched), acc


def _side_wgrads(plan, sched):
    return [p for p, (i, lane) in enumerate(sched) if lane > 0 and plan.bwd[i].type == "wgrad"]


def test_catches_a_wgrad_in_front_of_its_dz(base):
    plan, dn, sched, acc = base
    hit = None
    for p in _side_wgrads(plan, sched):
        dz = plan.bwd[sched[p][0]].a["dz"]
        for q in range(p):
            if sched[q][1] == 0 and any(n == dz.t and m == "w" and lo < dz.co + 96 and hi > dz.co for n, lo, hi, m in acc[q]):
                hit = (p, q, dz.t)
    assert hit is not None, "no side-lane weight gradient reads a gradient the main lane writes"
    p, q, name = hit
    bad = sched[:q] + [sched[p]] + sched[q:p] + sched[p + 1:]        # the wgrad directly in front of the op that writes its dz
    assert ("WAR", q, q + 1, name) in LM.hazards(plan, bad)
    assert (q, q + 1, name) in LM.unordered_writers(plan, bad)


def test_catches_a_reduction_on_another_lane_than_its_wgrad(base):
    plan, dn, sched, acc = base
    p = _side_wgrads(plan, sched)[0]
    slab = plan.bwd[sched[p][0]].a["slab"]
    r = next(k for k, (i, lane) in enumerate(sched) if plan.bwd[i].type == "wreduce" and plan.bwd[i].a["slab"] == slab)
    assert sched[p][1] == 1 and sched[r][1] == 1 and p < r
    bad = list(sched)
    bad[p] = (sched[p][0], 3)                                        # lanes 1 and 3 are not ordered
    found = LM.hazards(plan, bad)
    assert ("RAW", p, r, slab) in found and all(f[0] == "RAW" and f[1] == p for f in found)


def test_catches_a_destination_aliased_onto_a_side_lane_operand(base):
    plan, dn, sched, acc = base
    p = _side_wgrads(plan, sched)[0]
    src = plan.bwd[sched[p][0]].a["src0"]
    q = next(k for k in range(p + 1, len(sched)) if sched[k][1] == 0 and plan.bwd[sched[k][0]].type == "conv" and
             all(plan.bwd[sched[k][0]].a.get(key) is None for key in ("unrot", "upsum", "urot", "dst32")))
    ops = list(plan.bwd)
    ops[sched[q][0]] = copy.deepcopy(ops[sched[q][0]])
    ops[sched[q][0]].a["dst"] = View(src.t, src.co)
    found = LM.hazards(plan, sched, ops)
    assert ("WAR", p, q, src.t) in found
    assert not LM.hazards(plan, sched), "the plan's own ops are untouched"


def test_catches_a_dropped_bucket_mark(base):
    plan, dn, sched, acc = base
    good, ol, mark_at = _events_sched(plan, dn)
    assert not LM.hazards(plan, good)
    lanes_of = {}
    for pos, (lane, ks) in mark_at.items():
        for k in ks:
            lanes_of.setdefault(k, set()).add(lane)
    k = next(k for k, lanes in sorted(lanes_of.items()) if len(lanes) > 1)      # a bucket whose reductions ran on two lanes
    lane = max(lanes_of[k])
    bad, _, _ = _events_sched(plan, dn, drop=(k, lane))
    found = LM.hazards(plan, bad)
    ext = [p for p, e in enumerate(bad) if e[0] == "ext"]
    assert found and all(f[0] == "RAW" and f[3] == "grads" and f[2] in ext for f in found)
    lo, hi = bucket_ranges(plan.layers, plan.nparams, plan.nparams)[k]
    assert all(bad[f[1]][1] == lane and plan.bwd[bad[f[1]][0]].type == "wreduce" and bad[f[2]][1][0][1:3] == (lo, hi) for f in found)
