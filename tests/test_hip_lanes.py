"""GPU: the executor's half of the lane contract (include/ssdn_hip.h, the comment on `ssdn_op`; csrc/api.hip::ssdn_run_ops) as ordering
litmus tests.  Hand-built lists of SSDN_OP_ACCUM / SSDN_OP_ZERO / SSDN_OP_EVENT_RECORD on fp32 buffers that hold small integers, so every
expected value is exact:

    producer   a chain of k  ACCUM X += ONES  over a large buffer (still running when an unordered consumer would start)
    consumer   ACCUM Y += X  on the lane under test  ->  Y == k in every element, compared on the device

No device-wide wait stands between producer and consumer; whatever synchronisation a test needs is issued after the consumer.  A broken
executor shows up as a wrong integer: every access is inside a live allocation.

Whether the buffers are large enough for that is decided once per run by a CONTROL: the same consumer on lane 3 reading what lane 1
produces -- two lanes the contract leaves unordered.  The control asserts nothing; its outcome, the size chosen and the producer's duration
go to lanes_litmus.txt in the suite's output directory (OUTDIR of tests/test_hip_ops.py; DESIGN.md section 2 quotes them)."""
import os

import pytest
import torch

import optim_ref as O
from test_hip_ops import OUTDIR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
K = 4                   # producer chain length
FILL = 256              # floats of a filler op
NEVENTS = 256           # csrc/api.hip: SSDN_NEVENTS, the executor's event ring


def _accum(dst, src, lane, n=None):
    from ssdn.hip import lib as L
    return ("accum", L.AccumArgs(dst.data_ptr(), src.data_ptr(), dst.numel() if n is None else n), lane)


def _zero(t, lane):
    from ssdn.hip import lib as L
    return ("zero", L.ZeroArgs(t.data_ptr(), t.numel() * t.element_size()), lane)


def _mark(handle, lane):
    from ssdn.hip import lib as L
    return ("event_record", L.EventArgs(handle), lane)


def _enqueue(recs, stream):
    """one ssdn_run_ops call; nothing waits.  (the returned list owns the argument structs)"""
    from ssdn.hip.engine import OpList
    ol = OpList(recs)
    ol.run(stream)
    return ol


def _stale(Y, want):
    return int((Y != want).sum().item())


def _note(line):
    os.makedirs(OUTDIR, exist_ok=True)
    with open(os.path.join(OUTDIR, "lanes_litmus.txt"), "a") as f:
        f.write(line + "\n")
    print(line)


@pytest.fixture(scope="module")
def big():
    """the large buffers, at the smallest size at which the control races (2^26 floats upwards, 2^28 at most)"""
    out = None
    for log2 in (26, 27, 28):
        out = None
        torch.cuda.empty_cache()
        n = 1 << log2
        ones = torch.ones(n, device=DEV)
        X, Y = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        # the producer's duration, alone on the device
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        _enqueue([_accum(X, ones, 0) for _ in range(K)], 0)                      # (warm-up: first launch of the kernel)
        torch.cuda.synchronize()
        t0.record()
        keep = _enqueue([_accum(X, ones, 0) for _ in range(K)], 0)
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1)
        # the control: lanes 1 and 3 are not ordered
        X.zero_()
        Y.zero_()
        keep = _enqueue([_accum(X, ones, 1) for _ in range(K)] + [_accum(Y, X, 3)], 0)
        torch.cuda.synchronize()
        stale = _stale(Y, K)
        del keep
        _note("buffers of 2^%d floats: producer of %d ACCUMs %.3f ms (%.3f ms each, %.0f GB/s); control raced: %d stale elements" %
              (log2, K, ms, ms / K, 3 * 4 * n * K / ms / 1e6, stale))
        out = dict(n=n, ones=ones, X=X, Y=Y, teeth=stale > 0, ms_each=ms / K)
        if stale > 0:
            break
    if not out["teeth"]:
        _note("the control never raced: the litmus tests below check values, but cannot tell an unordered consumer from an ordered one")
    yield out
    del out
    torch.cuda.empty_cache()


@pytest.fixture(params=["null", "stream"])
def caller(request, big):
    """the caller's stream: the null stream, or a torch.cuda.Stream made current -> its raw handle"""
    if request.param == "null":
        assert torch.cuda.current_stream().cuda_stream == 0
        yield 0
    else:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            yield s.cuda_stream
    torch.cuda.synchronize()


def _fresh(big):
    """X = Y = 0, enqueued on the caller's (current) stream: work the list has to be ordered after"""
    big["X"].zero_()
    big["Y"].zero_()
    return big["ones"], big["X"], big["Y"]


# ---- C1: lanes 1 and 3 see the lane-0 ops in front of them, and what the caller enqueued before the call --------------------------------
@pytest.mark.parametrize("lane", [1, 3])
def test_c1_side_lanes_see_preceding_main_lane_ops(big, caller, lane):
    ones, X, Y = _fresh(big)
    keep = _enqueue([_accum(X, ones, 0) for _ in range(K)] + [_accum(Y, X, lane)], caller)
    torch.cuda.synchronize()
    assert _stale(Y, K) == 0 and _stale(X, K) == 0
    del keep


@pytest.mark.parametrize("lane", [1, 3])
def test_c1_side_lanes_see_the_callers_earlier_work(big, caller, lane):
    ones, X, Y = _fresh(big)
    for _ in range(K):
        X.add_(ones)                                 # torch ops on the caller's stream, enqueued before the call
    keep = _enqueue([_accum(Y, X, lane)], caller)
    torch.cuda.synchronize()
    assert _stale(Y, K) == 0
    del keep


# ---- C2: lane 2 sees the preceding ops of lanes 0, 1 and 3 --------------------------------------------------------------------------------
@pytest.mark.parametrize("src", [0, 1, 3])
def test_c2_lane_2_sees_lanes_0_1_and_3(big, caller, src):
    ones, X, Y = _fresh(big)
    keep = _enqueue([_accum(X, ones, src) for _ in range(K)] + [_accum(Y, X, 2)], caller)
    torch.cuda.synchronize()
    assert _stale(Y, K) == 0
    del keep


# ---- C3: same-lane order on each side lane -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lane", [1, 2, 3])
def test_c3_a_side_lane_runs_in_list_order(big, caller, lane):
    ones, X, Y = _fresh(big)
    keep = _enqueue([_accum(X, ones, lane) for _ in range(K)] + [_accum(Y, X, lane), _zero(X, lane), _accum(X, Y, lane)], caller)
    torch.cuda.synchronize()
    assert _stale(Y, K) == 0 and _stale(X, K) == 0
    del keep


# ---- C4: the join ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("consumer", ["torch", "second_call"])
@pytest.mark.parametrize("lane", [1, 2, 3])
def test_c4_join_behind_a_plain_accum(big, caller, lane, consumer):
    """after the call returns, work enqueued on the caller's stream sees the side lane's result; the only wait is the read-back"""
    ones, X, Y = _fresh(big)
    keep = [_enqueue([_accum(X, ones, lane) for _ in range(K)], caller)]
    if consumer == "torch":
        Y.add_(X)
    else:
        keep.append(_enqueue([_accum(Y, X, 0)], caller))
    stale = _stale(Y, K)                             # (a torch reduction on the caller's stream, then the host waits for that stream)
    torch.cuda.synchronize()
    assert stale == 0
    del keep


def _reductions():
    from test_hip_grad_accum import _Red
    cfgs = [(8, 0, True, 0, 0.3), (70, 1, False, 12, None), (40, 0, True, 12, 0.3)]      # nslabs <= 32 and > 32, tapblock, gb NULL, c_off
    return [_Red(900 + i, ns, tb, wb, co, inv) for i, (ns, tb, wb, co, inv) in enumerate(cfgs)]


@pytest.mark.parametrize("consumer", ["torch", "second_call"])
def test_c4_join_behind_a_merged_reduction_run(big, caller, consumer):
    """the last side-lane op is a merged run of SSDN_OP_WREDUCE on lane 2, queued behind the long producer: its last launch carries the
    join's stop event.  What the caller's stream copies right after the call is wreduce_ref's exact result."""
    ones, X, Y = _fresh(big)
    items = _reductions()
    for it in items:
        it.reset("nan", 0)
    sink = [torch.zeros_like(it.gw) for it in items]
    keep = [_enqueue([_accum(X, ones, 2) for _ in range(K)] + [("wreduce", it.args, 2) for it in items], caller)]
    if consumer == "torch":
        got = [it.gw.clone() for it in items]
    else:
        for s in sink:
            s.fill_(0.0)
        # (NaN + 0 stays NaN: the elements the op does not write stay recognisable)
        keep.append(_enqueue([_accum(s, it.gw, 0) for s, it in zip(sink, items)], caller))
        got = sink
    got = [g.cpu() for g in got]
    torch.cuda.synchronize()
    for it, g in zip(items, got):
        inv = None if it.inv is None else float(it.inv.cpu()[0])
        r = O.wreduce_ref(it.slab0.cpu(), it.bslab.cpu(), it.args, inv=inv, with_bias=it.with_bias)
        wr = ~torch.isnan(r["w32"])
        assert int(wr.sum()) > 0 and torch.equal(torch.isnan(g), ~wr), "the reduction's writes had not arrived"
        if consumer == "torch":
            assert torch.equal(g[wr].view(torch.int32), r["w32"][wr].view(torch.int32))
        else:
            assert torch.equal(g[wr], r["w32"][wr] + 0.0)
    del keep


@pytest.mark.parametrize("consumer", ["torch", "second_call"])
def test_c4_join_behind_the_fused_tail(big, caller, consumer):
    """... and that run followed by SSDN_OP_ADAM + its re-packs -- one k_tail_fused launch -- on lane 2, with the lists of
    tests/test_hip_tail_fused.py: the caller's stream reads the state the same records leave on the main lane"""
    from test_hip_optimiser import LR
    from test_hip_tail_fused import _Tail, _hostile, _same
    ones, X, Y = _fresh(big)
    layers, entries = _hostile()
    tl = _Tail(layers, entries, 781)
    red, opt = tl.recs(O.adam_args(LR, 5, 1.0))
    tl.reset()
    keep = [_enqueue(red + opt, caller)]
    torch.cuda.synchronize()
    want, want_changed = tl.state(), tl.slabs_changed()
    assert not any(want_changed), "the list did not run as the fused launch"
    g_model, _ = tl.model_gradient()
    assert torch.equal(torch.from_numpy(want["g"])[:tl.n].view(torch.int32), g_model[:tl.n].view(torch.int32))
    tl.reset()
    keep.append(_enqueue([_accum(X, ones, 2) for _ in range(K)] + [(t, a, 2) for t, a in red + opt], caller))
    if consumer == "second_call":
        probe = torch.zeros(tl.n, device=DEV)
        keep.append(_enqueue([_accum(probe, tl.p, 0, n=tl.n)], caller))
        probe = probe.cpu().numpy()
    got = tl.state()                                 # (copies on the caller's stream; the host waits for each)
    changed = tl.slabs_changed()
    torch.cuda.synchronize()
    assert not any(changed)
    _same(got, want, "fused tail on lane 2 against lane 0")
    if consumer == "second_call":
        assert (probe == want["p"][:tl.n] + 0.0).all()
    del keep


# ---- C5: an event mark stands for its lane's prefix ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("lane", [0, 1, 2, 3])
def test_c5_a_stream_that_waits_for_a_mark_sees_the_lanes_prefix(big, caller, lane):
    """lane 0 produces X (K adds); lane `lane` folds it into Y and adds K more; the mark follows on that lane.  A stream that waits for the
    mark must see Y == 2 K: the lane's earlier ops and the lane-0 ops those waited for.  The handle is made the way ssdn/hip/dp.py does."""
    ones, X, Y = _fresh(big)
    ev = torch.cuda.Event(enable_timing=False, blocking=False)
    ev.record(torch.cuda.current_stream())          # creates the underlying hipEvent_t (complete at once: a mark that is never recorded shows)
    waiter = torch.cuda.Stream()
    out = torch.zeros_like(Y)
    waiter.wait_stream(torch.cuda.current_stream())
    recs = [_accum(X, ones, 0) for _ in range(K)] + [_accum(Y, X, lane)] + [_accum(Y, ones, lane) for _ in range(K)] + \
        [_mark(int(ev.cuda_event), lane)]
    keep = _enqueue(recs, caller)
    waiter.wait_event(ev)
    with torch.cuda.stream(waiter):
        out.add_(Y)
    waiter.synchronize()
    stale = _stale(out, 2 * K)
    torch.cuda.synchronize()
    assert stale == 0
    del keep


# ---- C6: more hand-offs than the event ring has slots --------------------------------------------------------------------------------------
def _fillers(lanes, pairs):
    """`pairs` rounds of tiny ops on the lanes given in turn: every change of lane to one that depends on the previous draws a ring event"""
    f = [torch.zeros(FILL, device=DEV) for _ in lanes]
    one = torch.ones(FILL, device=DEV)
    recs = []
    for _ in range(pairs):
        for t, lane in zip(f, lanes):
            recs.append(_accum(t, one, lane))
    return recs, f, one


LONG_K = 32 * K        # a producer that outlasts the host's enqueueing of ~600 fillers (measured: 3.5 - 5.3 ms; 128 ACCUMs over 2^26 floats ~20 ms)


@pytest.mark.parametrize("end", ["lane2", "join"])
def test_c6_a_covered_side_lane_survives_the_ring_wrap(big, caller, end):
    """ADVICE round 3.  Lane 1 produces X and ends in a slab reduction: the LAST op of a side lane carries the join's stop event, so lane 1
    is covered by a ring event that nobody has waited for yet.  NEVENTS + 44 hand-offs main lane -> lane 3 then hand that slot out again,
    to an event recorded on the main lane -- which is not ordered behind lane 1.  (i) a later lane-2 consumer and (ii) the join must still
    wait for lane 1 itself.  lanes_litmus.txt (OUTDIR) says whether the producer outlasted the enqueueing."""
    import time
    ones, X, Y = _fresh(big)
    fill, f, one = _fillers((0, 3), NEVENTS + 44)
    red = _reductions()[0]
    red.reset("nan", 0)
    recs = [_accum(X, ones, 1) for _ in range(LONG_K)] + [("wreduce", red.args, 1)] + fill
    t0 = time.perf_counter()
    if end == "lane2":
        keep = _enqueue(recs + [_accum(Y, X, 2)], caller)
    else:
        keep = _enqueue(recs, caller)
        Y.add_(X)
    host_ms = 1e3 * (time.perf_counter() - t0)
    stale = _stale(Y, LONG_K)
    gw = red.gw.cpu()
    torch.cuda.synchronize()
    _note("ring wrap (%s), lane-1 producer of %d ACCUMs over 2^%d floats (~%.1f ms): the host enqueued list and consumer in %.2f ms" %
          (end, LONG_K, big["n"].bit_length() - 1, LONG_K * big["ms_each"], host_ms))
    assert stale == 0
    r = O.wreduce_ref(red.slab0.cpu(), red.bslab.cpu(), red.args, inv=float(red.inv.cpu()[0]), with_bias=red.with_bias)
    wr = ~torch.isnan(r["w32"])
    assert torch.equal(torch.isnan(gw), ~wr) and torch.equal(gw[wr].view(torch.int32), r["w32"][wr].view(torch.int32))
    assert all(_stale(t, NEVENTS + 44) == 0 for t in f)
    del keep


def test_c6_the_main_lanes_cover_survives_the_ring_wrap(big, caller):
    """the same wrap with the MAIN lane covered: the first lane-1 filler waits for the producer, lanes 1 -> 2 hand over NEVENTS + 44 times
    without new main-lane work, then lane 3 -- which has not waited for the main lane yet -- consumes.  (Here a stale slot has been
    re-recorded behind work that itself waited for the producer, so this pins the bookkeeping across the wrap, not the round-3 bug.)"""
    ones, X, Y = _fresh(big)
    fill, f, one = _fillers((1, 2), NEVENTS + 44)
    keep = _enqueue([_accum(X, ones, 0) for _ in range(LONG_K)] + fill + [_accum(Y, X, 3)], caller)
    torch.cuda.synchronize()
    assert _stale(Y, LONG_K) == 0
    assert all(_stale(t, NEVENTS + 44) == 0 for t in f)
    del keep
