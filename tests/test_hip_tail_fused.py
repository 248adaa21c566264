"""k_tail_fused (csrc/tail_fused.hip): a run of SSDN_OP_WREDUCE directly followed by SSDN_OP_ADAM and its run of SSDN_OP_WPACK as ONE
launch -- bit for bit what the three present launches (k_wreduce_partial_multi, k_wreduce_multi, k_adam_pack) leave, with the slabs only
read.  The same records run as one list (fuses) and as two lists (reductions | Adam + re-packs: cannot fuse); the host models of
tests/optim_ref.py say what both must give."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import optim_ref as O
from test_hip_optimiser import DEV, GUARD, LR, SENT, _adam_struct, _bits, _check_adam, _layer, _run

pytestmark = pytest.mark.gpu

INV = 0.3           # a non-power-of-two inv_scale


def _entry(layer, nslabs, m_off=0, M=None, c_off=0, cin=None, Kpad=None, bias=True, inv=None):
    return SimpleNamespace(layer=layer, nslabs=nslabs, m_off=m_off, M=M, c_off=c_off, cin=cin, Kpad=Kpad, bias=bias, inv=inv)


def _slab_values(gen, shape):
    """fp32 slabs with every kind of value the summation order can be told by: magnitudes over 12 decades, -0.0, subnormals, and pairs
    +-x of magnitude up to 1e30 in neighbouring slabs of one element (they cancel in the chain -- and swallow whatever the chain held
    before them, so the result depends on the order -- and leave a gradient Adam can square)"""
    ns = shape[0]
    x = (torch.randint(0, 2, shape, generator=gen).float() * 2 - 1) * 10.0 ** (torch.rand(shape, generator=gen) * 12 - 9)
    r = torch.rand(shape, generator=gen)
    x[r < 0.02] = -0.0
    sub = (r >= 0.02) & (r < 0.04)
    x[sub] = (torch.randint(-(1 << 22), 1 << 22, shape, generator=gen).float() * 2.0 ** -149)[sub]
    if ns >= 2:
        flat = x.reshape(ns, -1)
        n = flat.shape[1]
        cols = torch.nonzero(torch.rand(n, generator=gen) < 0.03).reshape(-1)
        s = torch.randint(0, ns - 1, (len(cols),), generator=gen)
        big = (torch.randint(0, 2, (len(cols),), generator=gen).float() * 2 - 1) * 10.0 ** (torch.rand(len(cols), generator=gen) * 20 + 10)
        flat[s, cols] = big
        flat[s + 1, cols] = -big
    return x


class _Tail:
    """[gap of 5 | W0 | b0 | W1 | b1 | ... | one lone float | tail gap ending mid-block] in one flat buffer; `entries` are the pending
    reductions (each with slabs of its own), layers without one keep the gradient the buffer was filled with."""

    def __init__(self, layers, entries, seed, accumulate=0):
        self.layers, self.entries, self.accumulate = layers, entries, accumulate
        off, self.w_off, self.b_off = 5, [], []
        for l in layers:
            self.w_off.append(off)
            off += l.M * l.cin * l.ntaps
            self.b_off.append(off)
            off += l.M
        off += 1 + 1024 + 517                         # the lone float and a gap that ends mid-block
        self.n = off
        p, g, m, v = O.adam_inputs(self.n + GUARD, seed)
        self.start = [torch.from_numpy(x) for x in (p, g, m, v)]
        self.p, self.g, self.m, self.v = (t.to(DEV) for t in self.start)
        self.shadows = []
        for l in layers:
            d = {"wf": torch.empty(l.ntaps * l.Mpad_f * l.Ktot, dtype=torch.int16, device=DEV)}
            if l.cm_f:
                d["wfc"] = torch.empty_like(d["wf"])
            if l.need_d:
                d["wd"] = torch.empty(l.ntaps * l.Mpad_d * l.Kd, dtype=torch.int16, device=DEV)
                if l.cm_d:
                    d["wdc"] = torch.empty_like(d["wd"])
            self.shadows.append(d)
        gen = torch.Generator().manual_seed(seed + 1)
        self.inv = torch.tensor([INV], dtype=torch.float32, device=DEV)
        c32 = lambda x: (x + 31) // 32 * 32          # noqa: E731
        for e in entries:
            l = layers[e.layer]
            e.M = l.M - e.m_off if e.M is None else e.M
            e.cin = l.cin - e.c_off if e.cin is None else e.cin
            e.Mpad = c32(e.M)
            e.Kpad = c32(e.cin) if e.Kpad is None else e.Kpad
            e.slab0 = _slab_values(gen, (e.nslabs, l.ntaps, e.Mpad, e.Kpad))
            e.bslab0 = _slab_values(gen, (e.nslabs, e.Mpad))
            e.slab, e.bslab = e.slab0.to(DEV), e.bslab0.to(DEV)
            e.args = SimpleNamespace(nslabs=e.nslabs, ntaps=l.ntaps, M=e.M, Mpad=e.Mpad, Kpad=e.Kpad, cin=e.cin, cin_full=l.cin,
                                     m_off=e.m_off, c_off=e.c_off, tapblock=0, accumulate=accumulate)

    def reset(self):
        for t, s in zip((self.p, self.g, self.m, self.v), self.start):
            t.copy_(s)
        for d in self.shadows:
            for t in d.values():
                t.fill_(SENT)
        for e in self.entries:
            e.slab.copy_(e.slab0)
            e.bslab.copy_(e.bslab0)

    def recs(self, args):
        from ssdn.hip import lib as L
        red = []
        for e in self.entries:
            a = e.args
            gw = self.g.data_ptr() + 4 * self.w_off[e.layer]
            gb = self.g.data_ptr() + 4 * self.b_off[e.layer] if e.bias else None
            red.append(("wreduce", L.WreduceArgs(e.slab.data_ptr(), e.bslab.data_ptr(), a.nslabs, a.ntaps, a.M, a.Mpad, a.Kpad, a.cin, a.cin_full,
                                                 a.m_off, a.c_off, 0, gw, gb, self.inv.data_ptr() if e.inv is not None else None, self.accumulate)))
        opt = [("adam", _adam_struct(self.p, self.g, self.m, self.v, self.n, args))]
        for i, (l, d) in enumerate(zip(self.layers, self.shadows)):
            ptr = lambda k: d[k].data_ptr() if k in d else None          # noqa: E731
            opt.append(("wpack", L.WpackArgs(self.p.data_ptr() + 4 * self.w_off[i], ptr("wf"), ptr("wd"), l.M, l.cin, l.ntaps, l.c0, l.c1_real,
                                             l.Mpad_f, l.Ktot, l.Mpad_d, l.Kd, ptr("wfc"), ptr("wdc"))))
        return red, opt

    def state(self):
        out = {k: getattr(self, k).cpu().numpy().copy() for k in "gpmv"}
        for i, d in enumerate(self.shadows):
            for k, t in d.items():
                out["%s%d" % (k, i)] = t.cpu().numpy().copy()
        return out

    def slabs_changed(self):
        """per entry: the weight slabs differ from what they were filled with; no bias slab may ever"""
        for e in self.entries:
            assert torch.equal(_bits(e.bslab), _bits(e.bslab0))
        return [not torch.equal(_bits(e.slab), _bits(e.slab0)) for e in self.entries]

    def model_gradient(self):
        """the flat gradient after the reductions by wreduce_ref's exact fp32 model, and a float64 check of it against `got`"""
        g = self.start[1].clone()
        checks = []
        for e in self.entries:
            l = self.layers[e.layer]
            w0, b0 = self.w_off[e.layer], self.b_off[e.layer]
            nw, nb = (e.m_off + e.M) * l.cin * l.ntaps, e.m_off + e.M
            r = O.wreduce_ref(e.slab0, e.bslab0, e.args, inv=e.inv, with_bias=e.bias, gw0=g[w0:w0 + nw].clone(), gb0=g[b0:b0 + nb].clone())
            for key, lo, cnt in (("w", w0, nw), ("b", b0, nb)):
                wr = ~torch.isnan(r[key + "32"])
                assert key == "b" and not e.bias or int(wr.sum()) > 0
                g[lo:lo + cnt][wr] = r[key + "32"][wr]
                checks.append((lo, wr, r[key + "64"], r[key + "_bound"]))
        return g, checks


def _same(a, b, what):
    for k in a:
        x, y = a[k].view(np.int16 if a[k].dtype == np.int16 else np.int32), b[k].view(np.int16 if b[k].dtype == np.int16 else np.int32)
        assert np.array_equal(x, y), "%s: %s differs in %d elements" % (what, k, int((x != y).sum()))


def _both_ways(tl, args):
    """the records as ONE list, then as two lists from the same state -> (state, slabs changed) of each"""
    red, opt = tl.recs(args)
    tl.reset()
    _run(red + opt)
    one = (tl.state(), tl.slabs_changed())
    tl.reset()
    _run(red)
    _run(opt)
    two = (tl.state(), tl.slabs_changed())
    return one, two


def _hostile():
    """ layer                                   entries (nslabs)
      0  M 16, cin 96 + 3, 9 taps               c_off 0 cin 96 (33, inv, bias) | c_off 96 cin 3, Kpad 16 (8)        split along the input channels
      1  M 24, cin 48, 9 taps                   m_off 0 M 16 (70, bias) | m_off 16 M 8 (65, inv)                    split along the output channels
      2  M 40, cin 48 + 16, 1 tap               (64, inv, bias)
      3  M 9,  cin 3, 9 taps, no wd             none: its gradient is what the buffer holds
      4  M 20, cin 12, 9 taps                   (1, bias)                                                          M % 8 != 0
      5  M 16, cin 96, 1 tap                    (32, bias)
      6  M 48, cin 96 + 48, 9 taps, chunk-major c_off 0 cin 96 (8, inv, bias) | c_off 96 cin 48 (32)
    Above 18 slabs a 9-tap tile is cut into quarters: entries of both kinds on both sides of every group boundary."""
    layers = [_layer(16, 99, 9, 96, 3, 112, 96, True, True, True),
              _layer(24, 48, 9, 48, 0, 48, 64, True, True, False),
              _layer(40, 64, 1, 48, 16, 64, 32, True, True, True),
              _layer(9, 3, 9, 0, 3, 16, 32, False, False, False),
              _layer(20, 12, 9, 12, 0, 16, 32, True, False, False),
              _layer(16, 96, 1, 96, 0, 96, 96, True, False, False),
              _layer(48, 144, 9, 96, 48, 144, 160, True, True, True)]
    entries = [_entry(0, 33, cin=96, inv=INV), _entry(0, 8, c_off=96, cin=3, Kpad=16, bias=False),
               _entry(1, 70, M=16), _entry(1, 65, m_off=16, M=8, bias=False, inv=INV),
               _entry(2, 64, inv=INV), _entry(4, 1), _entry(5, 32),
               _entry(6, 8, cin=96, inv=INV), _entry(6, 32, c_off=96, cin=48, bias=False)]
    return layers, entries


def test_fused_tail_on_a_hostile_layout():
    layers, entries = _hostile()
    assert sorted(e.nslabs for e in entries) == [1, 8, 8, 32, 32, 33, 64, 65, 70]
    tl = _Tail(layers, entries, 777)
    args = O.adam_args(LR, 7, 1.0 / 3.0)
    (one, one_changed), (two, two_changed) = _both_ways(tl, args)
    # 1. bit for bit the unfused result: gw, gb, p, m, v, every shadow, the guard behind n
    _same(one, two, "fused against unfused")
    p0, g0, m0, v0 = (t.numpy() for t in tl.start)
    n = tl.n
    for k, was in (("g", g0), ("p", p0), ("m", m0), ("v", v0)):
        assert np.array_equal(one[k][n:].view(np.int32), was[n:].view(np.int32)), k
    # 2. the fused launch only reads the slabs; stage 1 of the unfused route overwrites the first slab of every group above 32 slabs
    assert not any(one_changed), one_changed
    assert two_changed == [e.nslabs > 32 for e in entries], two_changed
    # 3. the host models: the reductions' documented order, bit for bit and within the float64 bound; nothing else of g written
    g_model, checks = tl.model_gradient()
    got_g = torch.from_numpy(one["g"])
    assert torch.equal(_bits(got_g[:n]), _bits(g_model[:n])), "%d gradient elements differ from the documented order" % \
        int((_bits(got_g[:n]) != _bits(g_model[:n])).sum())
    for lo, wr, m64, bound in checks:
        err = (got_g[lo:lo + len(wr)][wr].double() - m64[wr]).abs()
        assert bool((err <= bound[wr]).all())
    untouched = torch.ones(n, dtype=torch.bool)
    for lo, wr, _, _ in checks:
        untouched[lo:lo + len(wr)][wr] = False
    assert int(untouched.sum()) > 1500 and torch.equal(_bits(got_g[:n][untouched]), _bits(tl.start[1][:n][untouched]))
    # ... Adam on that gradient within the float64 bounds
    gq = one["g"][:n]
    assert np.isfinite(gq).all() and float(np.abs(gq).max()) < 1e19
    _check_adam("k_tail_fused on the hostile layout", one["p"][:n], one["m"][:n], one["v"][:n], p0[:n], gq, m0[:n], v0[:n], args)
    mod = O.adam_model32(p0[:n], gq, m0[:n], v0[:n], args)              # (diagnostic, as in test_hip_optimiser: its fma double-rounds)
    print("elements that differ from the float32 model: " + ", ".join("%s %d" % (k, int((one[k][:n] != mod[k]).sum())) for k in "mvp"))
    # ... and every shadow is wpack_ref of the new parameters at the real positions, the padding never written
    for i, l in enumerate(layers):
        W = one["p"][tl.w_off[i]:tl.w_off[i] + l.M * l.cin * l.ntaps]
        want = O.wpack_ref(W, l, need_d=l.need_d, cm_f=l.cm_f, cm_d=l.cm_d)
        assert set(want) == set(tl.shadows[i])
        for k, (vals, real) in want.items():
            got = torch.from_numpy(one["%s%d" % (k, i)])
            assert torch.equal(got[real], vals[real]), "layer %d %s: %d real elements differ" % (i, k, int((got[real] != vals[real]).sum()))
            assert bool((got[~real] == SENT).all()), "layer %d %s: padding written" % (i, k)


def test_fused_tail_is_repeatable():
    """the launch leaves the slabs as they were: a second run of the list from the same optimiser state gives the same bits"""
    layers, entries = _hostile()
    tl = _Tail(layers, entries, 778)
    args = O.adam_args(LR, 3, 1.0)
    red, opt = tl.recs(args)
    tl.reset()
    _run(red + opt)
    first = tl.state()
    for t, s in zip((tl.p, tl.g, tl.m, tl.v), tl.start):
        t.copy_(s)
    _run(red + opt)
    _same(first, tl.state(), "second run")


@pytest.mark.parametrize("why", ["accumulate", "misaligned"])
def test_lists_that_must_not_fuse(why):
    """accumulate = 1 (the epilogue adds to the old gradient), and an entry that starts at input channel 16 of a 64-channel layer (a
    48-channel tile would belong to two entries): the present kernels serve the list -- same bits as the two-list form, stage 1's
    overwrite of the slabs included"""
    if why == "accumulate":
        layers, entries = _hostile()
        tl = _Tail(layers, entries, 779, accumulate=1)
    else:
        layers = [_layer(16, 64, 9, 48, 16, 64, 64, True, True, True), _layer(8, 48, 1, 48, 0, 48, 64, True, False, False)]
        entries = [_entry(0, 33, cin=16, inv=INV), _entry(0, 40, c_off=16, cin=48, bias=False), _entry(1, 8)]
        tl = _Tail(layers, entries, 780)
    (one, one_changed), (two, two_changed) = _both_ways(tl, O.adam_args(LR, 2, 1.0))
    _same(one, two, why)
    assert one_changed == two_changed == [e.nslabs > 32 for e in entries]
    assert any(one_changed)
    g_model, _ = tl.model_gradient()
    assert torch.equal(_bits(torch.from_numpy(one["g"])[:tl.n]), _bits(g_model[:tl.n]))


@pytest.mark.parametrize("mode", ["known", "var"])
def test_train_step_with_and_without_the_deferred_tail(mode, monkeypatch):
    """The real engine at its smallest: with DEFER_TAIL (as shipped) the step's last reductions stand directly in front of Adam and the
    list fuses; without it they close the backward list, Adam stands in a list of its own and nothing fuses.  Mode var: two Adam ranges,
    only the first has a tail in front of it.  Parameters, gradient and moments bit-identical after every step."""
    import ssdn.hip.engine as E
    from test_hip_denoiser_autograd import batch, seeded_denoiser
    assert E.DEFER_TAIL is True
    data = [batch("ssdn", "gauss25", 3, 2, 32, seed=s) for s in range(3)]
    runs = []
    for defer in (True, False):
        monkeypatch.setattr(E, "DEFER_TAIL", defer)
        d = seeded_denoiser("ssdn", "gauss25", mode, 3)
        steps = []
        for b in data:
            d.train_step(b, 3e-4)
            torch.cuda.synchronize()
            steps.append([t.detach().clone() for t in (d.flat, d.flat_grad, d.adam_m, d.adam_v)])
        eng = d._last_train_engine
        assert eng.ops_opt_tail is not None and len(eng._adam_args) == (2 if mode == "var" else 1)
        runs.append(steps)
    for i, (a, b) in enumerate(zip(*runs)):
        for nm, x, y in zip(("flat", "flat_grad", "adam_m", "adam_v"), a, b):
            assert torch.equal(_bits(x), _bits(y)), "step %d: %s differs in %d elements" % (i + 1, nm, int((_bits(x) != _bits(y)).sum()))
    assert not torch.equal(runs[0][0][0], runs[0][2][0])
