"""GPU: the optimiser side of a training step -- SSDN_OP_WREDUCE, SSDN_OP_ADAM, SSDN_OP_WPACK and the fused k_adam_pack launch
(csrc/elementwise.hip) -- against the float64 references and exact host models of tests/optim_ref.py (checked on their own in
tests/test_optim_ref_cpu.py).

Adam: every element of p, m and v within FACTOR = 2 times the first-order rounding bounds of optim_ref.adam_ref64 plus one fp32 subnormal
spacing -- bounds counted from the kernel's operations, never taken from a measurement.  The 16-bit shadows and the slab reductions are
compared bit for bit.  Each test appends its worst error / bound ratios to optimiser_bounds.txt in the suite's output directory."""
import itertools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import optim_ref as O
from test_hip_ops import OUTDIR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LR = 3e-4
GUARD = 64


def _record(line):
    os.makedirs(OUTDIR, exist_ok=True)
    with open(os.path.join(OUTDIR, "optimiser_bounds.txt"), "a") as f:
        f.write(line + "\n")
    print(line)


def _struct_args(a):
    """the fp32 values an ssdn_adam_args struct carries"""
    return SimpleNamespace(**{k: np.float32(getattr(a, k)) for k in ("lr", "b1", "b2", "eps", "bc1", "bc2", "gscale")})


def _adam_struct(p, g, m, v, n, args, off=0):
    from ssdn.hip import lib as L
    return L.AdamArgs(p.data_ptr() + 4 * off, g.data_ptr() + 4 * off, m.data_ptr() + 4 * off, v.data_ptr() + 4 * off, n,
                      float(args.lr), float(args.b1), float(args.b2), float(args.eps), float(args.bc1), float(args.bc2), float(args.gscale))


def _run(recs):
    from ssdn.hip.engine import OpList, current_stream
    OpList(recs).run(current_stream())
    torch.cuda.synchronize()


def _check_adam(what, got_p, got_m, got_v, p, g, m, v, args):
    """every element of the device's p, m, v against adam_ref64 of the start state -> the worst ratios"""
    ref = O.adam_ref64(p, g, m, v, args)
    r = O.adam_ratios(got_p, got_m, got_v, ref)
    _record("%s: error / bound  m %.4f  v %.4f  p %.4f   (allowed %.1f)" % (what, r["m"], r["v"], r["p"], O.FACTOR))
    if max(r.values()) > O.FACTOR:
        mod = O.adam_model32(p, g, m, v, args)                           # diagnostic only
        for k, got in (("m", got_m), ("v", got_v), ("p", got_p)):
            err = np.abs(np.asarray(got).astype(np.float64) - ref[k])
            bad = err > O.FACTOR * ref["E_" + k] + O.TINY
            print("%s %s: %d of %d elements outside the bound, %d differ from the float32 model" %
                  (what, k, int(bad.sum()), bad.size, int((np.asarray(got) != mod[k]).sum())))
    assert r["m"] <= O.FACTOR and r["v"] <= O.FACTOR and r["p"] <= O.FACTOR, (what, r)
    return r


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).reshape(-1) if t.element_size() == 2 else t.detach().cpu().contiguous().view(torch.int32).reshape(-1)


# ---- (a) SSDN_OP_ADAM alone: k_adam ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [1, 2, 10, 1000, 100000])
@pytest.mark.parametrize("n", [1, 255, 257, 100003, 524288 + 4099])
def test_adam_op_vs_float64(n, step):
    """One step from a given state (step 1: m = v = 0).  n = 524288 + 4099 is past 2048 blocks of 256 threads: the second trip of the
    grid-stride loop.  g must stay as it is, and so must the elements behind n."""
    worst = dict(m=0.0, v=0.0, p=0.0)
    for gi, gscale in enumerate((1.0, 0.25, 1.0 / 3.0)):
        p, g, m, v = O.adam_inputs(n + GUARD, 1000 * step + 10 * gi + n % 7, zero_moments=step == 1)
        dp, dg, dm, dv = (torch.from_numpy(x).to(DEV) for x in (p, g, m, v))
        args = O.adam_args(LR, step, gscale)
        s = _adam_struct(dp, dg, dm, dv, n, args)
        assert _struct_args(s).__dict__ == args.__dict__
        _run([("adam", s)])
        gp, gg, gm, gv = (t.cpu().numpy() for t in (dp, dg, dm, dv))
        r = _check_adam("k_adam n=%d step=%d gscale=%.4f" % (n, step, gscale), gp[:n], gm[:n], gv[:n], p[:n], g[:n], m[:n], v[:n], args)
        worst = {k: max(worst[k], r[k]) for k in worst}
        assert np.array_equal(gg.view(np.int32), g.view(np.int32))                                   # g untouched
        for got, was in ((gp, p), (gm, m), (gv, v)):
            assert np.array_equal(got[n:].view(np.int32), was[n:].view(np.int32))                    # the guard behind n
        assert not np.array_equal(gp[:n], p[:n]) or n == 1
    _record("k_adam n=%d step=%d WORST over gscale: m %.4f v %.4f p %.4f" % (n, step, worst["m"], worst["v"], worst["p"]))


# ---- (b) the fused route on a layout built to break it ------------------------------------------------------------------------------------
SENT = 0x5A5A          # sentinel bit pattern of the shadows (fp16 205.25 / bf16 1.5e16: no weight of the test comes near)


def _layer(M, cin, ntaps, c0, c1_real, Ktot, Mpad_d, need_d, cm_f, cm_d):
    c = lambda x, q: (x + q - 1) // q * q                 # noqa: E731
    return SimpleNamespace(M=M, cin=cin, ntaps=ntaps, c0=c0, c1_real=c1_real, Mpad_f=c(M, 32), Ktot=Ktot, Mpad_d=Mpad_d, Kd=c(M, 16),
                           need_d=need_d, cm_f=cm_f, cm_d=cm_d)


class _Layout:
    """[gap of 5 | W0 | b0 | W1 | one lone float | W2 | b2 | W3 | tail gap ending mid-block] in one flat buffer, pads by the planner's rules
    (ssdn/hip/graph.py: Mpad a multiple of 32, Ktot / Kd multiples of 16):
      W0  M 9,  cin 3,  9 taps: the first layer's shape (c0 = 0, 3 real of 16 slots), no data-gradient shadow
      W1  M 20, cin 12, 9 taps: M % 8 != 0, cin % 48 != 0, 12 real of 16 slots
      W2  M 96, c0 96 + c1_real 48: Ktot 144, three chunks; chunk-major copies of both shadows
      W3  M 48, cin 64 = 48 + 16 (the tail chunk), 1 tap, chunk-major copies, and a data-gradient shadow of only 32 of the 64 input slots
          (decode_block_1.0 is planned so: its image channels need no gradient, Mpad_d < Ktot)"""

    def __init__(self):
        self.layers = [_layer(9, 3, 9, 0, 3, 16, 32, False, False, False),
                       _layer(20, 12, 9, 12, 0, 16, 32, True, False, False),
                       _layer(96, 144, 9, 96, 48, 144, 160, True, True, True),
                       _layer(48, 64, 1, 48, 16, 64, 32, True, True, True)]
        off, self.w_off = 5, []
        for l, extra in zip(self.layers, (9, 1, 96, 1024 + 517)):            # b0 | the lone float | b2 | the tail gap (ends mid-block)
            self.w_off.append(off)
            off += l.M * l.cin * l.ntaps + extra
        self.n = off
        p, g, m, v = O.adam_inputs(self.n + GUARD, 4242)
        self.start = [torch.from_numpy(x) for x in (p, g, m, v)]
        self.p, self.g, self.m, self.v = (t.to(DEV) for t in self.start)
        self.shadows = []
        for l in self.layers:
            d = {"wf": torch.empty(l.ntaps * l.Mpad_f * l.Ktot, dtype=torch.int16, device=DEV)}
            if l.cm_f:
                d["wfc"] = torch.empty_like(d["wf"])
            if l.need_d:
                d["wd"] = torch.empty(l.ntaps * l.Mpad_d * l.Kd, dtype=torch.int16, device=DEV)
                if l.cm_d:
                    d["wdc"] = torch.empty_like(d["wd"])
            self.shadows.append(d)

    def reset(self, state=True):
        if state:
            for t, s in zip((self.p, self.g, self.m, self.v), self.start):
                t.copy_(s)
        for d in self.shadows:
            for t in d.values():
                t.fill_(SENT)

    def wpack(self, i):
        from ssdn.hip import lib as L
        l, d = self.layers[i], self.shadows[i]
        ptr = lambda k: d[k].data_ptr() if k in d else None          # noqa: E731
        return ("wpack", L.WpackArgs(self.p.data_ptr() + 4 * self.w_off[i], ptr("wf"), ptr("wd"), l.M, l.cin, l.ntaps, l.c0, l.c1_real,
                                     l.Mpad_f, l.Ktot, l.Mpad_d, l.Kd, ptr("wfc"), ptr("wdc")))

    def state(self):
        return [t.cpu().numpy().copy() for t in (self.p, self.m, self.v)]

    def want(self, p_new, i):
        l = self.layers[i]
        W = p_new[self.w_off[i]:self.w_off[i] + l.M * l.cin * l.ntaps]
        return O.wpack_ref(W, l, need_d=l.need_d, cm_f=l.cm_f, cm_d=l.cm_d)

    def check_shadows(self, p_new, which, padding, what):
        """every shadow of the layers `which` bit-equal to wpack_ref of p_new at the real positions; the padding holds `padding`
        ("zero": what k_wpack writes, "sentinel": never touched by the fused launch)"""
        for i in which:
            want = self.want(p_new, i)
            assert set(want) == set(self.shadows[i])
            for k, (vals, real) in want.items():
                got = _bits(self.shadows[i][k])
                assert torch.equal(got[real], vals[real]), "%s: layer %d %s, %d real elements differ" % (what, i, k, int((got[real] != vals[real]).sum()))
                pad = got[~real]
                assert int(real.sum()) > 0                                       # (W2's forward shadow has no padding; every other has)
                if padding == "zero":
                    assert not bool(pad.any()), "%s: layer %d %s: padding not zeroed" % (what, i, k)
                    assert torch.equal(got, vals)
                else:
                    assert bool((pad == SENT).all()), "%s: layer %d %s: %d padding elements written" % (what, i, k, int((pad != SENT).sum()))


def test_fused_adam_pack_on_a_hostile_layout():
    lay = _Layout()
    args = O.adam_args(LR, 7, 1.0 / 3.0)
    p0, g0, m0, v0 = (t.numpy() for t in lay.start)
    n = lay.n
    adam = lambda lo=0, cnt=n: ("adam", _adam_struct(lay.p, lay.g, lay.m, lay.v, cnt, args, lo))      # noqa: E731

    # 1. plain SSDN_OP_ADAM, alone in its list: nothing to fuse
    lay.reset()
    _run([adam()])
    plain = lay.state()
    _check_adam("k_adam on the layout buffer", plain[0][:n], plain[1][:n], plain[2][:n], p0[:n], g0[:n], m0[:n], v0[:n], args)

    # 2. [adam, wpack x 4]: ONE k_adam_pack launch
    lay.reset()
    _run([adam()] + [lay.wpack(i) for i in range(4)])
    fused = lay.state()
    _check_adam("k_adam_pack on the layout buffer", fused[0][:n], fused[1][:n], fused[2][:n], p0[:n], g0[:n], m0[:n], v0[:n], args)
    for nm, x, y, was in zip("pmv", fused, plain, (p0, m0, v0)):
        assert np.array_equal(x.view(np.int32), y.view(np.int32)), "%s: %d elements differ from the unfused step" % (nm, int((x != y).sum()))
        assert np.array_equal(x[n:].view(np.int32), was[n:].view(np.int32)), nm                          # the guard behind the tail gap
    assert np.array_equal(lay.g.cpu().numpy().view(np.int32), g0.view(np.int32))
    p_new = fused[0]
    lay.check_shadows(p_new, range(4), "sentinel", "fused")       # (padding untouched: the documented behaviour, and the proof that the
    #                                                                 fused launch served the list)
    # 3. the four re-packs without the Adam op: k_wpack_multi; then each alone: k_wpack.  Padding zeroed.
    lay.reset(state=False)
    _run([lay.wpack(i) for i in range(4)])
    assert np.array_equal(lay.p.cpu().numpy().view(np.int32), p_new.view(np.int32))
    lay.check_shadows(p_new, range(4), "zero", "k_wpack_multi")
    for i in range(4):
        lay.reset(state=False)
        _run([lay.wpack(i)])
        lay.check_shadows(p_new, [i], "zero", "k_wpack")
        for j in range(4):
            if j != i:
                assert all(bool((t == SENT).all()) for t in lay.shadows[j].values())

    # 4. lists that must NOT fuse: re-packs out of order; a weight tensor outside the Adam range.  Same numbers by the unfused route.
    lay.reset()
    _run([adam()] + [lay.wpack(i) for i in (1, 0, 2, 3)])
    got = lay.state()
    for nm, x, y in zip("pmv", got, plain):
        assert np.array_equal(x.view(np.int32), y.view(np.int32)), nm
    lay.check_shadows(p_new, range(4), "zero", "out of order")
    lay.reset()
    cut = lay.w_off[3] + 100                                       # the range ends inside W3
    _run([adam(0, cut)] + [lay.wpack(i) for i in range(4)])
    got = lay.state()
    for nm, x, y, was in zip("pmv", got, plain, (p0, m0, v0)):
        assert np.array_equal(x[:cut].view(np.int32), y[:cut].view(np.int32)), nm
        assert np.array_equal(x[cut:].view(np.int32), was[cut:].view(np.int32)), nm
    lay.check_shadows(got[0], range(4), "zero", "outside the range")

    # 5. a range that starts inside the buffer (the second network's launch does): the leading gap is then W-relative, not 0-relative
    lay.reset()
    lo = lay.w_off[1] - 4                                          # the last 4 biases of b0 lead; W0 is outside and not in the list
    _run([adam(lo, n - lo)] + [lay.wpack(i) for i in (1, 2, 3)])
    got = lay.state()
    for nm, x, y, was in zip("pmv", got, plain, (p0, m0, v0)):
        assert np.array_equal(x[lo:].view(np.int32), y[lo:].view(np.int32)), nm
        assert np.array_equal(x[:lo].view(np.int32), was[:lo].view(np.int32)), nm
    lay.check_shadows(got[0], (1, 2, 3), "sentinel", "fused, range starting inside")
    assert all(bool((t == SENT).all()) for t in lay.shadows[0].values())


# ---- (c) the real layouts -------------------------------------------------------------------------------------------------------------------
def _real_denoiser(cfg):
    from test_hip_denoiser_autograd import seeded_denoiser
    from test_hip_diag_cov import diag_denoiser
    if cfg == "diag":
        return diag_denoiser("gauss25", "known", 3), "ssdn"
    alg, style, mode = cfg.split("/")
    return seeded_denoiser(alg, style, mode, 3), alg


@pytest.mark.parametrize("cfg", ["ssdn/gauss25/var", "n2c/gauss25/known", "diag"])
def test_engine_adam_on_the_real_layouts(cfg):
    """engine.adam() -- the launch every training step runs -- over the WHOLE flat buffer of real networks, with the gradient of one real
    backward pass, and every 16-bit shadow of every layer against wpack_ref of the new parameters.  A network that silently stopped
    fusing (ADAM_PACK_MAX) still has to be right."""
    from test_hip_denoiser_autograd import batch
    d, alg = _real_denoiser(cfg)
    d.run_pipeline(batch(alg, "gauss25", 3, 2, 32))
    d.backward()
    torch.cuda.synchronize()
    eng = d._last_train_engine
    nets = [eng.main] + ([eng.sigma] if eng.sigma is not None else [])
    assert len(eng._adam_args) == len(nets) == (2 if cfg.endswith("var") else 1)
    ntot = d.flat.numel()
    p0, g0 = d.flat.detach().cpu().numpy().copy(), d.flat_grad.detach().cpu().numpy().copy()
    assert np.isfinite(g0).all() and float(np.abs(g0).max()) > 0
    for step, gscale in ((1, 1.0), (7, 1.0 / 3.0)):
        if step == 1:
            m0, v0 = np.zeros(ntot, np.float32), np.zeros(ntot, np.float32)
        else:
            _, _, m0, v0 = O.adam_inputs(ntot, 99)
        with torch.no_grad():
            d.flat.copy_(torch.from_numpy(p0))
            d.adam_m.copy_(torch.from_numpy(m0))
            d.adam_v.copy_(torch.from_numpy(v0))
        eng.adam(LR, step, gscale)
        torch.cuda.synchronize()
        want = O.adam_args(LR, step, gscale)
        for a in eng._adam_args:
            assert _struct_args(a).__dict__ == want.__dict__
        assert sum(int(a.n) for a in eng._adam_args) == ntot
        gp, gm, gv = (t.detach().cpu().numpy().copy() for t in (d.flat, d.adam_m, d.adam_v))
        _check_adam("engine.adam %s step=%d gscale=%.4f" % (cfg, step, gscale), gp, gm, gv, p0, g0, m0, v0, want)
        assert np.array_equal(d.flat_grad.detach().cpu().numpy().view(np.int32), g0.view(np.int32))
        nsh = 0
        for net in nets:
            plan = net.plan
            for op in plan.pack:
                a = SimpleNamespace(**op.a)
                l = next(x for x in plan.layers if x.name == a.layer)
                w_off = plan.param_base + l.w_off
                ref = O.wpack_ref(gp[w_off:w_off + l.M * l.cin * l.ntaps], a, need_d=a.need_d, cm_f=a.cm_f, cm_d=a.cm_d)
                for k, (vals, real) in ref.items():
                    got = _bits(net.t[plan.prefix + k + "/" + a.layer])
                    assert torch.equal(got[real], vals[real]), (cfg, step, a.layer, k, int((got[real] != vals[real]).sum()))
                    assert not bool(got[~real].any()), (cfg, step, a.layer, k)        # the padding: the zeros of the first re-pack
                    nsh += 1
                for k in ("wd", "wfc", "wdc"):
                    assert (k in ref) == (plan.prefix + k + "/" + a.layer in net.t), (a.layer, k)
        assert nsh >= 50 * len(nets)


# ---- (d) SSDN_OP_WREDUCE --------------------------------------------------------------------------------------------------------------------
def _check_reduction(it, inv, accumulate, what):
    """the device's gw / gb of a finished run of `it` (a test_hip_grad_accum._Red) against optim_ref.wreduce_ref -> worst error / bound"""
    r = O.wreduce_ref(it.slab0.cpu(), it.bslab.cpu(), it.args, inv=inv, with_bias=it.with_bias, gw0=it.P_w.cpu(), gb0=it.P_b.cpu())
    worst = 0.0
    for k, got, before in (("w", it.gw.cpu(), it.P_w.cpu() if accumulate else None), ("b", it.gb.cpu(), it.P_b.cpu() if accumulate else None)):
        m32, m64, B = r[k + "32"], r[k + "64"], r[k + "_bound"]
        wr = ~torch.isnan(m32)
        assert k == "b" and not it.with_bias or int(wr.sum()) > 0
        err = (got[wr].double() - m64[wr]).abs()
        assert bool((err <= B[wr]).all()), "%s %s: %d elements outside the float64 bound" % (what, k, int((err > B[wr]).sum()))
        if err.numel():
            worst = max(worst, float((err / B[wr]).max()))
        ndiff = int((_bits(got[wr]) != _bits(m32[wr])).sum())
        assert ndiff == 0, "%s %s: %d of %d elements differ from the documented summation order" % (what, k, ndiff, int(wr.sum()))
        if accumulate:
            assert torch.equal(_bits(got[~wr]), _bits(before[~wr])), "%s %s: wrote outside its block" % (what, k)
        else:
            assert bool(torch.isnan(got[~wr]).all()), "%s %s: wrote outside its block" % (what, k)
    return worst


@pytest.mark.parametrize("tapblock", [0, 1])
@pytest.mark.parametrize("nslabs", [1, 8, 32, 33, 64, 65, 70])
def test_wreduce_vs_float64_and_the_documented_order(nslabs, tapblock):
    """Single launches (k_wreduce_partial above 32 slabs, k_wreduce): within the float64 bound AND bit-equal to the exact fp32 model of the
    order the header documents -- weights in groups of 32 slabs, then the groups; the bias in one chain -- from NaN-filled (accumulate:
    pre-filled) gw / gb; nothing outside the block written.  32 / 33 is where stage 1 starts, 64 / 65 where a third group starts."""
    from ssdn.hip.engine import OpList, current_stream
    from test_hip_grad_accum import _Red
    worst = 0.0
    for i, (c_off, m_off, with_bias, inv, acc) in enumerate(itertools.product((0, 12), (0, 4), (True, False), (None, 0.3), (0, 1))):
        it = _Red(7000 + 100 * nslabs + i, nslabs, tapblock, with_bias, c_off, inv, m_off=m_off)
        it.reset("P" if acc else "nan", acc)
        OpList([("wreduce", it.args)]).run(current_stream())
        torch.cuda.synchronize()
        worst = max(worst, _check_reduction(it, inv, acc, "nslabs=%d tapblock=%d c_off=%d m_off=%d bias=%d inv=%s acc=%d" %
                                            (nslabs, tapblock, c_off, m_off, with_bias, inv, acc)))
    _record("k_wreduce nslabs=%d tapblock=%d: worst error / float64 bound %.4f (32 cases, all bit-equal to the fp32 model)" % (nslabs, tapblock, worst))


def test_wreduce_merged_run_of_five():
    """the same through k_wreduce_partial_multi + k_wreduce_multi: five entries in one run, mixed in every respect"""
    from ssdn.hip.engine import OpList, current_stream
    from test_hip_grad_accum import _Red
    cfgs = [(33, 0, True, 0, 0, None, 0), (70, 1, False, 12, 4, 0.3, 1), (32, 0, True, 12, 4, 0.3, 0), (65, 1, True, 0, 0, None, 1),
            (1, 0, False, 0, 4, 0.3, 1)]
    items = []
    for i, (ns, tb, wb, co, mo, inv, acc) in enumerate(cfgs):
        it = _Red(9000 + i, ns, tb, wb, co, inv, m_off=mo)
        it.reset("P" if acc else "nan", acc)
        items.append(it)
    OpList([("wreduce", it.args) for it in items]).run(current_stream())
    torch.cuda.synchronize()
    worst = max(_check_reduction(it, c[5], c[6], "merged entry %d" % i) for i, (it, c) in enumerate(zip(items, cfgs)))
    _record("k_wreduce_multi run of five: worst error / float64 bound %.4f (all bit-equal to the fp32 model)" % worst)
