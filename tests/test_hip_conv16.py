"""GPU: k_conv16 (csrc/conv16.hip) -- the 96-channel 3x3 layers at 16x16 pixels on a resident half-image tile.

Every launch of the class runs twice from the same NaN-poisoned buffers: on k_conv16 (ssdn_conv_set_conv16(3)) and on the path it
replaces, k_conv's flat path (ssdn_conv_set_conv16(0)).  All outputs must agree bit for bit -- the kernel keeps k_conv's accumulation
order, MFMA instruction and operand roles, and its epilogue arithmetic -- and lie within the teacher-forced bounds of
tests/test_hip_ops.py::test_every_op_teacher_forced of a float64 convolution of the same 16-bit operands.  Launches outside the class
(32x32 pixels, 99 input channels, 48 output channels, fp32 output) must be refused by the predicate and stay what they were; one
Denoiser.train_step with the kernel on and off must leave the same bits everywhere.

The plans hold these launches with the flags used here: forward bias + LeakyReLU; data gradient with the fp16 activation as LeakyReLU' mask
(no launch of k_conv's reads sign bytes: ssdn_conv_signs refuses them, here as before), with the skip addend, and -- decode_block_3.0's --
with the fused SSDN_OP_UPSUM_BWD output, which the library only fuses into a launch without mask and addend (ssdn_conv_fuses_upsum)."""
import pytest
import torch

from conv_case import Case, _check_ref, _same      # the launch builder, its float64 reference and the bit comparison

pytestmark = pytest.mark.gpu


def _lib():
    from ssdn.hip import lib as L
    return L, L.load()


@pytest.fixture(autouse=True)
def conv16_reset():
    yield
    L, lib = _lib()
    lib.ssdn_conv_set_conv16(-1)
    lib.ssdn_conv_set_mode(1)


def _taps(name):
    from ssdn.hip import graph
    return graph.TAPS_BLIND if name == "blind" else graph.TAPS_PLAIN


# (role, c0, c1, up0, M, mask, add, upsum_c): the four launches of decode_block_3.0 / 3.2, and the data gradient with mask AND addend
LAUNCHES = {
    "fwd_96_96": ("fwd", 96, 0, False, 96, False, False, 0),
    "fwd_144up_96": ("fwd", 96, 48, True, 96, False, False, 0),
    "dgrad_96_96_mask": ("dgrad", 96, 0, False, 96, True, False, 0),
    "dgrad_96_144_upsum": ("dgrad", 96, 0, False, 144, False, False, 96),
    "dgrad_96_96_mask_add": ("dgrad", 96, 0, False, 96, True, True, 0),
}


def _both(case, what):
    L, lib = _lib()
    L.check(lib.ssdn_conv_set_conv16(3))
    assert case.eligible() == 1, "%s: not claimed by ssdn_conv16_eligible" % what
    new = case.run(3)
    assert case.eligible() == 1
    old = case.run(0)
    assert case.eligible() == 0, "%s: the switch does not reach the old path" % what
    _same(new, old, what)
    return new


@pytest.mark.parametrize("name,taps", [(n, "blind") for n in LAUNCHES] + [("fwd_144up_96", "plain"), ("dgrad_96_144_upsum", "plain")])
def test_conv16_against_k_conv_and_float64(name, taps):
    """N = 3: image and half indices that are no power of two, and a last workgroup group that is partly void.  TAPS_PLAIN once per role."""
    role, c0, c1, up0, M, mask, add, uc = LAUNCHES[name]
    case = Case(role, 3, c0, c1, up0, M, _taps(taps), mask=mask, add=add, upsum_c=uc, seed=len(name))
    _check_ref(case, _both(case, name))


@pytest.mark.parametrize("name", ["fwd_96_96", "fwd_144up_96", "dgrad_96_96_mask", "dgrad_96_144_upsum"])
def test_conv16_chunk_major_weights(name):
    """the plans hand these launches the chunk-major copy of the weights too, and k_conv16 streams from it (contiguous slices); k_conv's
    flat path reads the plain shadow.  Same bits."""
    role, c0, c1, up0, M, mask, add, uc = LAUNCHES[name]
    case = Case(role, 3, c0, c1, up0, M, _taps("blind"), mask=mask, add=add, upsum_c=uc, seed=31, cm=True)
    _check_ref(case, _both(case, name + " (chunk-major weights)"))


@pytest.mark.parametrize("name", ["fwd_144up_96", "dgrad_96_144_upsum", "dgrad_96_96_mask"])
def test_conv16_halo_zero_fill(name):
    """Inputs that are zero except next to the borders the halo zero-fills: rows 0 and 1 in the forward role (the blind-spot window reaches
    two rows up), the last two rows in the data gradient (it reaches two rows down), columns 0 and 15.  A fill that starts a row or a
    column off multiplies exactly these values."""
    role, c0, c1, up0, M, mask, add, uc = LAUNCHES[name]
    case = Case(role, 3, c0, c1, up0, M, _taps("blind"), mask=mask, add=add, upsum_c=uc, seed=77, edge=True)
    _check_ref(case, _both(case, name + " (border values only)"), sparse=True)


@pytest.mark.parametrize("name", ["fwd_96_96", "dgrad_96_144_upsum"])
def test_conv16_single_image(name):
    role, c0, c1, up0, M, mask, add, uc = LAUNCHES[name]
    case = Case(role, 1, c0, c1, up0, M, _taps("blind"), mask=mask, add=add, upsum_c=uc, seed=5)
    _check_ref(case, _both(case, name + " N = 1"))


FALLBACKS = {
    "32x32": dict(role="fwd", N=1, c0=96, c1=0, up0=False, M=96, H=32, W=32),
    "99_channels": dict(role="fwd", N=3, c0=96, c1=16, up0=False, M=96),          # 99 real channels in 112 slots: no whole 48-channel chunks
    "48_outputs": dict(role="fwd", N=3, c0=96, c1=0, up0=False, M=48),
    "dst32": dict(role="fwd", N=3, c0=96, c1=0, up0=False, M=9, dst32=True),
}


@pytest.mark.parametrize("name", list(FALLBACKS))
def test_conv16_refuses_what_is_not_its_class(name):
    """the predicate says no with the kernel switched on, and the launch gives what it gives with the kernel switched off"""
    case = Case(taps=_taps("blind"), seed=11, **FALLBACKS[name])
    L, lib = _lib()
    L.check(lib.ssdn_conv_set_conv16(3))
    assert case.eligible() == 0
    new, old = case.run(3), case.run(0)
    _same(new, old, name)
    key = "dst32" if "dst32" in new else "dst"
    body = new[key] if key == "dst32" else new[key][..., 8:8 + case.M]
    assert bool(torch.isfinite(body.float()).all())


def _train_step_state(roles, accumulate):
    import restate as R
    import ssdn
    from ssdn.denoiser import Denoiser
    from ssdn.datasets import NoisyDataset
    from ssdn.params import ConfigValue, NoiseAlgorithm, NoiseValue
    L, lib = _lib()
    L.check(lib.ssdn_conv_set_conv16(roles))
    cfg = ssdn.cfg.base()
    cfg[ConfigValue.ALGORITHM] = NoiseAlgorithm.SELFSUPERVISED_DENOISING
    cfg[ConfigValue.NOISE_STYLE] = "gauss25"
    cfg[ConfigValue.NOISE_VALUE] = NoiseValue.KNOWN
    ssdn.cfg.infer(cfg, model_only=True)
    d = Denoiser(cfg, device="cuda:0")
    d.get_model(Denoiser.MODEL, parallelised=False).load_state_dict(R.reference_state_dict(R.make_params(3, 9, True, seed=5)))
    d.mark_dirty()
    B, P = 2, 64
    d.train()
    out = None
    for k in range(2 if accumulate else 1):
        clean = R.hash_tensor((B, 3, P, P), 61 + 10 * k, 0, 1)
        noisy = torch.clamp(clean + R.hash_tensor((B, 3, P, P), 62 + 10 * k, -1, 1) * 0.17, 0, 1)
        meta = {NoisyDataset.Metadata.INPUT_NOISE_VALUES: torch.full((B, 1, 1, 1), 25 / 255.0), NoisyDataset.Metadata.CLEAN: clean}
        if accumulate and k == 0:
            d.accumulate_step([noisy, clean, meta])
        else:
            out = d.train_step([noisy, clean, meta], lr=3e-4)
    torch.cuda.synchronize()
    state = {"out/" + str(k): v.detach().cpu().clone() for k, v in out.items() if torch.is_tensor(v)}
    state["flat"] = d.flat.detach().cpu().clone()
    state["flat_grad"] = d.flat_grad.detach().cpu().clone()
    return state


@pytest.mark.parametrize("accumulate", [False, True])
def test_train_step_is_bit_identical_with_conv16_on_and_off(accumulate):
    """batch 2 at 64x64: 8 rotated images whose 16x16 stage is the kernel's class.  The returned dictionary, the flat gradient and the updated
    parameters; once with a micro-batch accumulated in front of the step."""
    on = _train_step_state(3, accumulate)
    off = _train_step_state(0, accumulate)
    assert len(on) >= 3
    _same(on, off, "train_step")
    assert bool(torch.isfinite(on["flat"]).all()) and float(on["flat_grad"].abs().max()) > 0
