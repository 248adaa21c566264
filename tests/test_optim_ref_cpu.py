"""CPU: the references of tests/optim_ref.py against each other and against the interpreter's own re-pack -- before
tests/test_hip_optimiser.py holds the device to them."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import optim_ref as O

N_CPU = 60_000            # (the float32 model was run once at n = 600 000: worst ratios 0.992 - 0.9996; this keeps the file at seconds)


# ---- Adam ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [1, 2, 10, 1000, 100000])
def test_float32_model_stays_within_the_float64_bounds(step):
    """adam_model32 (the kernel's operation order in numpy float32) within 1.0x of E_m, E_v, E_p on the inputs of the GPU test; and the
    inputs do what they are chosen for: a share of the elements in the regime that pins eps, the update visible in p."""
    for gscale in (1.0, 0.25, 1.0 / 3.0, 0.125):
        p, g, m, v = O.adam_inputs(N_CPU, 7 + step, zero_moments=step == 1)
        a = O.adam_args(3e-4, step, gscale)
        ref = O.adam_ref64(p, g, m, v, a)
        mod = O.adam_model32(p, g, m, v, a)
        r = O.adam_ratios(mod["p"], mod["m"], mod["v"], ref)
        print("step %d gscale %.4f: model / bound m %.4f v %.4f p %.4f" % (step, gscale, r["m"], r["v"], r["p"]))
        assert max(r.values()) <= 1.0, r
        den = np.sqrt(ref["v"]) / np.sqrt(float(a.bc2))
        share_eps = float(np.mean(den < 10 * float(a.eps)))
        share_vis = float(np.mean(np.abs(ref["p"] - p.astype(np.float64)) > 8 * O.U * np.abs(p)))
        assert 0.08 <= share_eps <= 0.5 and share_vis >= 0.9, (share_eps, share_vis)


def test_float64_reference_is_adam():
    """adam_ref64 against ONE step of torch.optim.Adam in float64 (betas (0.9, 0.99), eps 1e-8: the reference trainer's optimiser) from
    the same state, at optimiser steps 1 and 7: the formula, the bias corrections, the place of eps, gscale as a factor of the gradient.
    torch carries 1 - beta in double, the ABI carries the fp32 betas: about 1e-6 relative in the increments, so rtol 1e-5."""
    n = 4000
    for step, gscale in ((1, 1.0), (7, 1.0 / 3.0)):
        p32, g32, m32, v32 = O.adam_inputs(n, 5 + step, zero_moments=step == 1)
        a = O.adam_args(3e-4, step, gscale)
        r = O.adam_ref64(p32, g32, m32, v32, a)
        w = torch.nn.Parameter(torch.from_numpy(p32).double())
        opt = torch.optim.Adam([w], lr=float(a.lr), betas=(0.9, 0.99), eps=1e-8)
        opt.state[w] = dict(step=torch.tensor(float(step - 1)), exp_avg=torch.from_numpy(m32).double(),
                            exp_avg_sq=torch.from_numpy(v32).double())
        w.grad = torch.from_numpy(g32).double() * float(a.gscale)
        opt.step()
        st = opt.state[w]
        # (m' may cancel: the 6e-8 between 0.9f and 0.9 is measured against the addends, as the bounds are)
        G = np.abs(g32.astype(np.float64) * float(a.gscale))
        slack_m = 1e-6 * (0.9 * np.abs(m32.astype(np.float64)) + 0.1 * G)
        assert bool((np.abs(r["m"] - st["exp_avg"].numpy()) <= slack_m).all())
        np.testing.assert_allclose(r["v"], st["exp_avg_sq"].numpy(), rtol=1e-5, atol=0)
        upd, upd_t = r["p"] - p32.astype(np.float64), w.detach().numpy() - p32.astype(np.float64)
        den = np.sqrt(r["v"]) / np.sqrt(float(a.bc2)) + float(a.eps)
        assert bool((np.abs(upd - upd_t) <= 1e-5 * np.abs(upd_t) + float(a.lr) / float(a.bc1) * slack_m / den).all())
        assert float(np.abs(upd_t).max()) > 1e-4
        # gscale is visible at more than the bound: a reference that dropped it would differ
        if gscale != 1.0:
            r1 = O.adam_ref64(p32, g32, m32, v32, O.adam_args(3e-4, step, 1.0))
            assert float(np.mean(np.abs(r1["p"] - r["p"]) > 4 * r["E_p"])) > 0.5
    # the kernel's 1 - b2 is 1.f - 0.99f, torch's is 0.01: about 1e-6 relative in v's increment
    rel = (1.0 - float(np.float32(0.99))) / 0.01 - 1.0
    assert 5e-7 < abs(rel) < 2e-6, rel


# ---- WREDUCE --------------------------------------------------------------------------------------------------------------------------------
def _red_args(nslabs, tapblock, c_off, m_off, accumulate):
    if tapblock:
        ntaps, M, Mpad, Kpad, cin = 3, 20, 32, 16, 40
    else:
        ntaps, M, Mpad, Kpad, cin = 9, 20, 32, 16, 12
    return SimpleNamespace(nslabs=nslabs, ntaps=ntaps, M=M, Mpad=Mpad, Kpad=Kpad, cin=cin, cin_full=c_off + cin + 4, m_off=m_off, c_off=c_off,
                           tapblock=int(tapblock), accumulate=int(accumulate))


@pytest.mark.parametrize("nslabs", [1, 8, 32, 33, 64, 65, 70])
def test_wreduce_fp32_model_stays_within_its_float64_bound(nslabs):
    gen = torch.Generator().manual_seed(nslabs)
    for tapblock in (0, 1):
        for c_off, m_off, with_bias, inv, acc in ((0, 0, True, None, 0), (12, 4, True, 0.3, 1), (12, 0, False, 0.3, 0), (0, 4, True, None, 1)):
            a = _red_args(nslabs, tapblock, c_off, m_off, acc)
            slab = torch.randn(nslabs, a.ntaps, a.Mpad, a.Kpad, generator=gen)
            bslab = torch.randn(nslabs, a.Mpad, generator=gen)
            nw = (m_off + a.M) * a.cin_full * (1 if tapblock else a.ntaps)
            gw0, gb0 = torch.randn(nw, generator=gen), torch.randn(m_off + a.M, generator=gen)
            r = O.wreduce_ref(slab, bslab, a, inv=inv, with_bias=with_bias, gw0=gw0, gb0=gb0)
            for k in ("w", "b"):
                m32, m64, B = r[k + "32"], r[k + "64"], r[k + "_bound"]
                wr = ~torch.isnan(m32)
                assert torch.equal(wr, ~torch.isnan(m64)) and torch.equal(wr, ~torch.isnan(B))
                assert bool(((m32[wr].double() - m64[wr]).abs() <= B[wr]).all())
            # what is written: M x cin real columns (x taps), the block's corner at (m_off, c_off); the bias only when gb is given
            wr = ~torch.isnan(r["w32"])
            assert int(wr.sum()) == a.M * a.cin * (1 if tapblock else a.ntaps)
            grid = wr.reshape(m_off + a.M, a.cin_full, -1)
            assert bool(grid[m_off:, c_off:c_off + a.cin].all()) and not bool(grid[:m_off].any()) and not bool(grid[:, :c_off].any())
            assert int((~torch.isnan(r["b32"])).sum()) == (a.M if with_bias else 0)


def test_wreduce_model_orders():
    """the order is visible: with 40 slabs the grouped sum (32 + 8) differs from the plain chain in some elements (with 33 the second
    group is one slab and the two orders are the same chain).  An element of the scatter, by hand."""
    gen = torch.Generator().manual_seed(1)
    a = _red_args(40, 0, 0, 0, 0)
    slab = torch.randn(40, a.ntaps, a.Mpad, a.Kpad, generator=gen)
    bslab = torch.randn(40, a.Mpad, generator=gen)
    r = O.wreduce_ref(slab, bslab, a)
    plain = O._seq_sum32([slab[s] for s in range(40)])
    grouped = (torch.zeros_like(slab[0]) + O._seq_sum32([slab[s] for s in range(32)])) + O._seq_sum32([slab[s] for s in range(32, 40)])
    t, m, k = 5, 7, 3
    assert float(r["w32"][(m * a.cin_full + k) * a.ntaps + t]) == float(grouped[t, m, k])
    assert not torch.equal(plain, grouped)
    assert float(r["b32"][m]) == float(O._seq_sum32([bslab[s] for s in range(40)])[m])
    a = _red_args(3, 1, 12, 4, 0)
    slab = torch.arange(3 * 3 * 32 * 16, dtype=torch.float32).reshape(3, 3, 32, 16)
    r = O.wreduce_ref(slab, torch.zeros(3, 32), a, with_bias=False)
    t, m, k = 2, 19, 7                                                     # channel 2 * 16 + 7 = 39 < 40
    assert float(r["w32"][(4 + m) * a.cin_full + 12 + 39]) == float(slab[:, t, m, k].sum())
    assert torch.isnan(r["w32"][(4 + m) * a.cin_full + 12 + 40])        # channel 40: padding of the last block


# ---- WPACK ----------------------------------------------------------------------------------------------------------------------------------
def _plans():
    from ssdn.hip.graph import NetPlan
    return [NetPlan("m/", 3, 9, True, 2, 32, 32, cus=8), NetPlan("s/", 3, 1, False, 2, 32, 32, cus=8)]


@pytest.mark.parametrize("which", [0, 1])
def test_wpack_ref_equals_the_interpreter_and_its_swizzle_inverts(which):
    """wf / wd of every layer of a blind-spot and a plain plan equal what oracle/interp.py packs (a second, independent restatement);
    wfc / wdc are permutations of wf / wd, and the inverse written from the storage side gives them back."""
    from interp import Interp
    plan = _plans()[which]
    gen = torch.Generator().manual_seed(11 + which)
    flat = torch.randn(plan.nparams, generator=gen) * 10.0 ** torch.randint(-6, 1, (plan.nparams,), generator=gen).float()
    it = Interp(plan, flat, fp16=True)
    it.run(plan.pack)
    n_cm = 0
    for op in plan.pack:
        a = SimpleNamespace(**op.a)
        l = it.L[a.layer]
        W = flat[l.w_off:l.w_off + l.M * l.cin * l.ntaps].numpy()
        r = O.wpack_ref(W, a, need_d=a.need_d, cm_f=a.cm_f, cm_d=a.cm_d)
        assert set(r) == {"wf"} | ({"wd"} if a.need_d else set()) | ({"wfc"} if a.cm_f else set()) | ({"wdc"} if a.cm_d else set())
        want_f = it.t[plan.prefix + "wf/" + a.layer].to(torch.float16).view(torch.int16).reshape(-1)
        assert torch.equal(r["wf"][0], want_f), a.layer
        assert int(r["wf"][1].sum()) == a.M * a.cin * a.ntaps
        assert not bool(r["wf"][0][~r["wf"][1]].any())                                               # padding: +0
        if a.need_d:
            want_d = it.t[plan.prefix + "wd/" + a.layer].to(torch.bfloat16).view(torch.int16).reshape(-1)
            assert torch.equal(r["wd"][0], want_d), a.layer
        for cm, rm, rows, K in (("wfc", "wf", a.Mpad_f, a.Ktot), ("wdc", "wd", a.Mpad_d, a.Kd)):
            if cm not in r:
                continue
            n_cm += 1
            assert torch.equal(torch.sort(r[cm][0])[0], torch.sort(r[rm][0])[0]), (a.layer, cm)      # a permutation
            assert int(r[cm][1].sum()) == int(r[rm][1].sum())
            back = O.chunk_major_undo(r[cm][0].numpy(), a.ntaps, rows, K)
            assert np.array_equal(back.reshape(-1), r[rm][0].numpy()), (a.layer, cm)
            backr = O.chunk_major_undo(r[cm][1].numpy(), a.ntaps, rows, K)
            assert np.array_equal(backr.reshape(-1), r[rm][1].numpy()), (a.layer, cm)
            if K > 8:
                assert not torch.equal(r[cm][0], r[rm][0])
    assert n_cm >= 20


def test_chunk_major_by_hand():
    """three places of the documented layout, worked out by hand for K = 64 (one chunk of 48, one of 16), 16 rows, 2 taps"""
    pos = O.chunk_major_positions(2, 16, 64)
    assert pos[0, 0, 0] == 0 and pos[0, 0, 47] == 47 and pos[0, 1, 0] == 48
    assert pos[0, 8, 0] == 8 * 48 + 8                   # row 8: pieces swap in pairs, piece 0 sits at piece 1
    assert pos[0, 8, 13] == 8 * 48 + 0 + 5              # ... and piece 1 at piece 0
    assert pos[0, 0, 48] == 48 * 16                     # the 16-wide tail chunk starts behind the 48-wide one: rows of 16
    assert pos[0, 9, 50] == 48 * 16 + 9 * 16 + 8 + 2    # row 9 of the tail: piece 0 at piece 1
    assert pos[1, 0, 0] == 16 * 64                      # taps outermost
    assert sorted(pos.reshape(-1).tolist()) == list(range(2 * 16 * 64))
