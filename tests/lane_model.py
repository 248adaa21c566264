"""TEST INFRASTRUCTURE -- the lane contract of include/ssdn_hip.h (the comment on `ssdn_op`) as a model, written from the header's text and not
from the executor (csrc/api.hip::ssdn_run_ops).  No tests in here: tests/test_lane_hazards_cpu.py uses it.

1. A HAPPENS-BEFORE relation over a list of items.  An item is an op on a lane, or one of three things the contract names besides ops:
     ("mark", lane)        SSDN_OP_EVENT_RECORD: stands for its OWN lane's prefix of the list (and what that prefix was ordered after);
     ("join",)             the end of one ssdn_run_ops call: every side lane is joined back into the caller's stream, and what a later call
                           enqueues -- on any lane -- is ordered after whatever the caller's stream held before it;
     ("ext", regions, waits)   a consumer outside the list (a gradient bucket's collective): ordered after exactly the marks at the
                           positions `waits`, touches `regions`.
   Op j is ordered after an earlier op i if they share a lane or i's lane is one j's lane depends on (DEPS), closed transitively.
2. An ACCESS TABLE: which region of which tensor an op of the planner (ssdn.hip.graph.Op) reads or writes.
3. hazards(): every pair of items that touch overlapping regions, at least one writing, without being ordered.

A region is (tensor, lo, hi, "r" | "w"); the unit of [lo, hi) is a property of the tensor:
   NHWC tensors ('act' / 'actb', always reached through a View)      channels
   slabs / bias slabs of a weight-gradient launch                      blocks (one per mblock)
   "params", "grads" (the owner's flat fp32 buffers)                  elements
   everything else (f32 images, weight shadows, sign bytes, route words, the scale word)   (0, WHOLE)
"""
from typing import List, Set, Tuple

WHOLE = 1 << 62
DEPS = {0: set(), 1: {0}, 3: {0}, 2: {0, 1, 3}}        # lanes a lane is ordered after (besides itself)


# ---- 2. the access table -----------------------------------------------------------------------------------------------------------------
def accesses(plan, op) -> Set[Tuple[str, int, int, str]]:
    """regions op touches, from the op's own arguments (include/ssdn_hip.h says what each argument struct reads and writes)"""
    a, P, base = op.a, plan.prefix, plan.param_base
    layer = {l.name: l for l in plan.layers}
    out = set()

    def view(key, width, mode, off=0):
        v = a.get(key)
        if v is not None and width > 0:
            out.add((v.t, v.co + off, v.co + off + width, mode))

    def named(name, mode, lo=0, hi=WHOLE):
        if name is not None:
            out.add((name, int(lo), int(hi), mode))

    def weights(lname, mode="r"):
        l = layer[lname]
        named("params", mode, base + l.w_off, base + l.w_off + l.M * l.cin * l.ntaps)

    t = op.type
    if t == "pack_input":
        named(a["src"], "r")
        view("dst", a["cpad"], "w")
    elif t == "conv":
        M, l = a["M"], layer[a["layer"]]
        view("src0", a["c0"], "r")
        view("src1", a["c1"], "r")
        fwd = a["role"] == "fwd"
        named(P + ("wf/" if fwd else "wd/") + a["layer"], "r")
        wc = P + ("wfc/" if fwd else "wdc/") + a["layer"]         # ssdn_conv_args.wc: the chunk-major copy, where the plan has one
        named(wc if wc in plan.tensors else None, "r")
        if a["bias"]:
            named("params", "r", base + l.b_off, base + l.b_off + M)
        if a["dst32"] is not None:                                # fp32 NCHW output: nothing else is applied
            named(a["dst32"], "w")
        elif a.get("urot") is not None:                           # fused SSDN_OP_UNROT_FWD: the only 16-bit output (+ sign bytes)
            view("urot", 4 * M, "w")
            named(a.get("urot_smask"), "w")
        else:
            view("add", M, "r")
            if a.get("mask_sign") is not None:                    # sign bytes stand in for the mask tensor
                named(a["mask_sign"], "r")
            else:
                view("mask", M, "r")
            if a.get("unrot") is not None:                        # fused SSDN_OP_UNROT_BWD: the launch's only output
                view("unrot", M // 4, "w")
                if a.get("unrot_smask") is not None:
                    named(a["unrot_smask"], "r")
                else:
                    view("unrot_mask", M // 4, "r")
            elif a.get("upsum") is not None:                      # fused SSDN_OP_UPSUM_BWD of the channels below upsum_c; the rest to dst
                c = a["upsum_c"]
                view("upsum", c, "w")
                if a.get("upsum_mask_sign") is not None:
                    named(a["upsum_mask_sign"], "r")
                else:
                    view("upsum_mask", c, "r")
                view("dst", M - c, "w", off=c)
            else:
                view("dst", M, "w")
                named(a.get("sign_out"), "w")
                view("pool", M, "w")
    elif t == "pool_fwd":
        view("act", a["C"], "r")
        view("pooled", a["C"], "w")
        named(a.get("route"), "w")
    elif t == "pool_bwd":
        view("dpool", a["C"], "r")
        view("dz", a["C"], "w")
        if a.get("route") is not None:                            # launched on its own it reads the route words instead of the activation
            named(a["route"], "r")
        else:
            view("act", a["C"], "r")
    elif t == "upsum_bwd":
        view("src", a["C"], "r")
        view("mask", a["C"], "r")
        view("dst", a["C"], "w")
    elif t == "unrot_fwd":
        view("src", a["C"], "r")
        view("dst", 4 * a["C"], "w")
        named(a.get("smask"), "w")
    elif t == "unrot_bwd":
        view("src", 4 * a["C"], "r")
        view("mask", a["C"], "r")
        view("dst", a["C"], "w")
    elif t == "grad_pack":
        named(a["g"], "r")
        view("dst", a["cpad"], "w")
        named(P + "scale", "w")                                   # scale_out: SSDN_OP_WREDUCE's inv_scale input
    elif t == "wgrad":
        mb = a.get("mblocks", 1)
        for b in range(mb):                                       # block b: dz channels [b M, b M + M) of the view
            view("dz", a["M"], "r", off=b * a["M"])
        view("src0", a["c0"], "r")
        view("src1", a["c1"], "r")
        named(a["slab"], "w", 0, mb)
        named(a["bslab"], "w", 0, mb)
    elif t == "wreduce":
        l, mb = layer[a["layer"]], a.get("mblock", 0)
        named(a["slab"], "r", mb, mb + 1)
        named(P + "scale", "r")
        for m in range(a["m_off"], a["m_off"] + a["M"]):          # gw[m][c_off .. c_off + cin)[all taps of the LAYER]
            lo = base + l.w_off + (m * a["cin_full"] + a["c_off"]) * l.ntaps
            named("grads", "w", lo, lo + a["cin"] * l.ntaps)
        if a["with_bias"]:
            named(a["bslab"], "r", mb, mb + 1)
            named("grads", "w", base + l.b_off + a["m_off"], base + l.b_off + a["m_off"] + a["M"])
    elif t == "wpack":
        l = a["layer"]
        weights(l)
        named(P + "wf/" + l, "w")
        named(P + "wd/" + l if a["need_d"] else None, "w")
        named(P + "wfc/" + l if a.get("cm_f") else None, "w")
        named(P + "wdc/" + l if a.get("cm_d") else None, "w")
    elif t == "input_grad":
        view("g_e0", 48, "r")
        view("g_d1a", 96, "r")
        named(a["dst"], "w")
        weights(a["layer_e"])
        weights(a["layer_d"])
    else:
        raise ValueError("lane_model.accesses: no entry for op type " + t)
    return out


# ---- 1. happens-before -------------------------------------------------------------------------------------------------------------------
class Item:
    def __init__(self, kind, lane=0, acc=(), waits=(), what=""):
        self.kind, self.lane, self.waits, self.what = kind, lane, tuple(waits), what
        by = {}                                                   # (tensor, mode) -> sorted disjoint intervals
        for name, lo, hi, mode in acc:
            by.setdefault((name, mode), []).append((lo, hi))
        for k, iv in by.items():
            iv.sort()
            merged = [iv[0]]
            for lo, hi in iv[1:]:
                if lo <= merged[-1][1]:
                    merged[-1] = (merged[-1][0], max(merged[-1][1], hi))
                else:
                    merged.append((lo, hi))
            by[k] = merged
        self.acc = by


def items_of(plan, sched, ops=None) -> List[Item]:
    """sched: (index into ops, lane) for an op -- ops: plan.bwd unless given --, or a ("mark", lane) / ("join",) / ("ext", regions, waits) entry"""
    ops = plan.bwd if ops is None else ops
    items = []
    for e in sched:
        if e[0] == "mark":
            items.append(Item("mark", e[1], what="mark on lane %d" % e[1]))
        elif e[0] == "join":
            items.append(Item("join", what="join"))
        elif e[0] == "ext":
            items.append(Item("ext", -1, e[1], e[2], what="outside consumer"))
        else:
            op = ops[e[0]]
            if e[1] not in DEPS:
                raise ValueError("bad lane %r" % (e[1],))
            items.append(Item("op", e[1], accesses(plan, op), what="%s %s (op %d, lane %d)" % (op.type, op.a.get("layer", ""), e[0], e[1])))
    return items


def happens_before(items) -> List[int]:
    """pred[j]: bit i set <=> item i is ordered before item j"""
    pred = []
    for j, it in enumerate(items):
        p = 0
        if it.kind == "join":
            p = (1 << j) - 1                                      # everything is ordered before "after the list"
        elif it.kind == "ext":
            for m in it.waits:
                if items[m].kind != "mark" or m >= j:
                    raise ValueError("an outside consumer waits for marks that precede it")
                p |= pred[m] | (1 << m)
        else:
            for i in range(j):
                a = items[i]
                if a.kind == "join":
                    direct = True
                elif a.kind == "ext":
                    direct = False
                elif it.kind == "mark":
                    direct = a.lane == it.lane                    # a mark waits for nothing: its own lane's prefix only
                else:
                    direct = a.lane == it.lane or a.lane in DEPS[it.lane]
                if direct:
                    p |= pred[i] | (1 << i)                       # (the transitive closure through the items in between)
        pred.append(p)
    return pred


# ---- 3. hazards --------------------------------------------------------------------------------------------------------------------------
def _overlap(x, y) -> bool:
    """two sorted lists of disjoint half-open intervals share a point"""
    i = j = 0
    while i < len(x) and j < len(y):
        if x[i][1] <= y[j][0]:
            i += 1
        elif y[j][1] <= x[i][0]:
            j += 1
        else:
            return True
    return False


def _touch(items):
    by = {}                                                       # tensor -> [(item index, mode, intervals)]
    for k, it in enumerate(items):
        for (name, mode), iv in it.acc.items():
            by.setdefault(name, []).append((k, mode, iv))
    return by


CLASS = {("w", "r"): "RAW", ("r", "w"): "WAR", ("w", "w"): "WAW"}


def hazards(plan, sched, ops=None):
    """-> sorted [(class, i, j, tensor)]: positions i < j of sched whose items overlap in a region of `tensor`, at least one writing, with i
    not ordered before j.  class by list order: RAW = i writes, j reads; WAR = i reads, j writes; WAW = both write."""
    items = items_of(plan, sched, ops)
    pred = happens_before(items)
    found = set()
    for name, accs in _touch(items).items():
        for y in range(len(accs)):
            j, mj, ivj = accs[y]
            for x in range(y):
                i, mi, ivi = accs[x]
                if i == j or (mi == "r" and mj == "r") or (pred[j] >> i) & 1:
                    continue
                if _overlap(ivi, ivj):
                    found.add((CLASS[(mi, mj)], i, j, name))
    return sorted(found)


def unordered_writers(plan, sched, ops=None):
    """The premise the header's guarantee leans on ("they read tensors written once per step"), as a check of its own: for every side-lane
    op, every region it READS has no writer anywhere in the list that is not ordered before that read.  -> [(reader, writer, tensor)]"""
    items = items_of(plan, sched, ops)
    pred = happens_before(items)
    bad = set()
    for name, accs in _touch(items).items():
        for j, mj, ivj in accs:
            if mj != "r" or items[j].kind != "op" or items[j].lane == 0:
                continue
            for i, mi, ivi in accs:
                if mi == "w" and i != j and not (pred[j] >> i) & 1 and _overlap(ivi, ivj):
                    bad.add((j, i, name))
    return sorted(bad)


def describe(plan, sched, found, ops=None) -> str:
    items = items_of(plan, sched, ops)
    return "\n".join("%s on %s: [%d] %s  <->  [%d] %s" % (f[0], f[3], f[1], items[f[1]].what, f[2], items[f[2]].what) for f in found)
