"""GPU tests of rtod_bn_grad (csrc/bn_grad.hip), the backward of batch-statistics BatchNorm, against exact integer results and the
numpy float64 model of tests/bn_grad_cases.py.

Gates, with u = 2^-24 and N = B H W.
* Small integers: du in -2..2, z in {-1, +1}, the mean handed to the kernel 0: S1 and S2 are integers below 2^53 in every order of
  summation, so dbeta is the integer sum and dgamma is float32(float64(S2) r) with numpy's r = 1 / sqrt(var + 1e-5): one correctly
  rounded double square root, division, product and one rounding to float on both sides, bit for bit.
* Floats: the kernel's sums are double sums of N terms in a tree (at most N - 1 roundings of 2^-53 each on a path, far fewer in
  fact), its dz a handful of double operations on them and one rounding to float:
      |dz - dz64| <= u |dz64| + N 2^-52 mass_dz,      |dgamma - dgamma64| <= u |dgamma64| + N 2^-53 sum |du (z - mean)| r,
      |dbeta - dbeta64| <= u |dbeta64| + N 2^-53 sum |du|
  with the masses of bn_grad_model (the sums of the absolute terms of each output).
* Every output is bit-identical on a second call."""
import numpy as np
import pytest
import torch

from bn_grad_cases import EPS, PARTS_SHAPE, SHAPES, U, batch_stats, bn_grad_model, float_case, integer_case
from realtimeobjectdetection_amd import train as T

pytestmark = pytest.mark.gpu
F = np.float32


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bn_grad(du, z, mean, var, gamma):
    out = T.bn_grad_async(_dev(du), _dev(z), _dev(np.asarray(mean, np.float64)), _dev(np.asarray(var, np.float64)), _dev(gamma))
    return tuple(t.cpu().numpy() for t in out)


@pytest.mark.parametrize("shape", SHAPES)
def test_bn_grad_exact_on_small_integers(shape):
    B, C_, H, W = shape
    du, z = integer_case(shape)
    var = np.linspace(0.5, 2.0, C_)
    gamma = np.ones(C_, F)
    dz, dgamma, dbeta = _bn_grad(du, z, np.zeros(C_), var, gamma)
    S1 = du.astype(np.float64).sum(axis=(0, 2, 3))
    S2 = (du.astype(np.float64) * z.astype(np.float64)).sum(axis=(0, 2, 3))
    r = 1.0 / np.sqrt(var + EPS)
    assert dbeta.tobytes() == S1.astype(F).tobytes(), shape
    assert dgamma.tobytes() == (S2 * r).astype(F).tobytes(), shape
    model = bn_grad_model(du, z, np.zeros(C_), var, gamma)              # exact sums: dz is a few double operations and one float rounding
    assert dz.shape == du.shape and (np.abs(dz - model[0]) <= U * np.abs(model[0]) + 2.0 ** -50 * model[3]).all(), shape


@pytest.mark.parametrize("shape", SHAPES)
def test_bn_grad_floats_within_the_double_sum_bound_and_reproducible(shape):
    B, C_, H, W = shape
    N = B * H * W
    du, z, gamma = float_case(shape)
    mean, var = batch_stats(z)
    got = _bn_grad(du, z, mean, var, gamma)
    want_dz, want_dg, want_db, m_dz, m_dg, m_db = bn_grad_model(du, z, mean, var, gamma)
    bounds = (U * np.abs(want_dz) + N * 2.0 ** -52 * m_dz, U * np.abs(want_dg) + N * 2.0 ** -53 * m_dg, U * np.abs(want_db) + N * 2.0 ** -53 * m_db)
    for name, g, w, bound in zip(("dz", "dgamma", "dbeta"), got, (want_dz, want_dg, want_db), bounds):
        err = np.abs(g.astype(np.float64) - w)
        print("bn_grad %s %s: worst error / bound %.3g" % (shape, name, float((err / bound).max())))
        assert g.dtype == F and g.shape == w.shape and (err <= bound).all(), (shape, name)
    again = _bn_grad(du, z, mean, var, gamma)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again)), shape


def test_bn_grad_ragged_shape_runs_several_parts():
    B, C_, H, W = PARTS_SHAPE
    parts, part_len = T.bn_grad_parts(B, C_, H * W)
    assert parts >= 3 and (B * H * W) % part_len != 0, (parts, part_len)


def test_bn_grad_takes_device_addresses_and_unaligned_views():
    """mean / var as the integer device addresses Darknet.bn_stats_dev hands out, and operands that are views at a 4-byte offset."""
    shape = SHAPES[0]
    du, z, gamma = float_case(shape, seed=1)
    mean, var = batch_stats(z)
    want = _bn_grad(du, z, mean, var, gamma)
    m, v = _dev(mean), _dev(var)
    pad = lambda a: torch.cat([torch.zeros(1, device="cuda"), _dev(a).reshape(-1)])[1:].view(a.shape)
    got = T.bn_grad_async(pad(du), pad(z), m.data_ptr(), v.data_ptr(), _dev(gamma))
    assert all(w.tobytes() == g.cpu().numpy().tobytes() for w, g in zip(want, got))


# ---------------------------------------------------------------------------------------------- the kept BatchNorm inputs of a plan
from bn_grad_cases import normalise_model, plan_stats  # noqa: E402
from realtimeobjectdetection_amd import cfgs  # noqa: E402
from realtimeobjectdetection_amd.cfg import build_ir  # noqa: E402
from scope_grad_cases import KEEP, _bn_of, _forward, _frames, _model  # noqa: E402


def _linear_cfg():
    """Stem, a LINEAR 1x1 BatchNorm conv, a leaky 3x3 one, a head: mini_cfg has no linear BatchNorm conv."""
    L = cfgs._net(64, 64) + cfgs._conv(32, 3, 1) + cfgs._conv(32, 1, 1, act="linear") + cfgs._conv(64, 3, 2)
    L += cfgs._conv(3 * 8, 1, 1, bn=False, act="linear") + cfgs._yolo((0, 1, 2), cfgs._ANCHORS_V3, 9, 3)
    return "\n".join(L) + "\n"


@pytest.mark.parametrize("name", ["mini", "linear"])
def test_forward_with_kept_bn_inputs_is_the_in_place_forward_and_read_bn_input_is_what_it_normalised(tmp_path, name):
    """At 64 x 64, batch 3, in .train() with the backbone's keep option, on mini_cfg and on a cfg with a linear BatchNorm conv.  The
    forward with keep_bn_inputs equals the forward without it bit for bit, output and every BatchNorm conv's stored map.
    read_bn_input(i) pushed through the forward's float expression with the plan's own statistics reproduces read_layer(i) bit for
    bit: on the first and the last leaky conv of the listing, and on the linear one."""
    text, B = (cfgs.mini_cfg(64, 64) if name == "mini" else _linear_cfg()), 3
    x = _frames(B, 64, None)
    kept = _model(tmp_path, text, 64, "fp32", dict(KEEP["backbone"], keep_bn_inputs=1), train=True, name="kept")
    # (without keep_bn_inputs a batch-statistics plan lists no conv and so keeps no activation: keep_all_layers makes its maps readable)
    plain = _model(tmp_path, text, 64, "fp32", KEEP["backbone"], train=True, keep_all=True, name="plain")
    y1, y0 = _forward(kept, x), _forward(plain, x)
    assert y1.cpu().numpy().tobytes() == y0.cpu().numpy().tobytes()
    listed = [c for c, _ in kept.trainable_layers()]
    assert listed and plain.trainable_layers() == []                  # without the option a batch-statistics plan trains nothing
    for c in listed:
        assert kept.read_layer(c, B).cpu().numpy().tobytes() == plain.read_layer(c, B).cpu().numpy().tobytes(), c
    with pytest.raises(Exception, match="keep_bn_inputs"):
        plain.read_bn_input(listed[0], B)
    ir = {L.index: L for L in build_ir(kept.blocks, 64).layers}
    leaky, linear = [c for c in listed if ir[c].leaky], [c for c in listed if not ir[c].leaky]
    assert leaky and (name == "mini" or linear == [1])
    for c in leaky[:1] + leaky[-1:] + linear[:1]:
        bn = _bn_of(kept, c)
        z = kept.read_bn_input(c, B).cpu().numpy()
        mean, var = plan_stats(kept, c, z.shape[1])
        want = normalise_model(z, mean, var, bn.weight.detach().cpu().numpy(), bn.bias.detach().cpu().numpy(), ir[c].leaky)
        assert kept.read_layer(c, B).cpu().numpy().tobytes() == want.tobytes(), c
        # the statistics are those of z: the plan's doubles against numpy's float64 mean / biased variance of the very tensor
        assert np.allclose(mean, z.astype(np.float64).mean(axis=(0, 2, 3)), rtol=0, atol=1e-12 * np.abs(z).max())
        assert (np.abs(var - z.astype(np.float64).var(axis=(0, 2, 3))) <= 1e-9 * (var + mean * mean)).all()     # (E[z^2] - mean^2 on the device)
