"""Host tests (no GPU) of the batch-statistics BatchNorm backward: the numpy float64 model of tests/bn_grad_cases.py against float64
torch autograd of F.batch_norm, the partition rule of rtod_bn_grad_parts, the workspace formula and the argument checks of the three
entries, all of which are decided before anything touches the device."""
import ctypes as C

import numpy as np
import pytest
import torch

from bn_grad_cases import PARTS_SHAPE, SHAPES, batch_stats, bn_grad_model, float_case
from realtimeobjectdetection_amd import _ffi

fn = torch.nn.functional


@pytest.mark.parametrize("shape", SHAPES)
def test_model_is_float64_autograd_of_batch_norm(shape):
    """Both are float64 sums of N terms: 8 N 2^-53 x the sum of the absolute terms of each output."""
    du, z, gamma = float_case(shape)
    B, C_, H, W = shape
    N = B * H * W
    mean, var = batch_stats(z)
    dz, dgamma, dbeta, m_dz, m_dgamma, m_dbeta = bn_grad_model(du, z, mean, var, gamma)
    zt = torch.from_numpy(z.astype(np.float64)).requires_grad_(True)
    gt = torch.from_numpy(gamma.astype(np.float64)).requires_grad_(True)
    bt = torch.zeros(C_, dtype=torch.float64, requires_grad=True)
    fn.batch_norm(zt, None, None, gt, bt, True, 0.0, 1e-5).backward(torch.from_numpy(du.astype(np.float64)))
    tol = 8 * N * 2.0 ** -53
    for name, got, want, mass in (("dz", dz, zt.grad.numpy(), m_dz), ("dgamma", dgamma, gt.grad.numpy(), m_dgamma), ("dbeta", dbeta, bt.grad.numpy(), m_dbeta)):
        worst = float((np.abs(got - want) / (tol * mass)).max())
        print("%s %s: worst error / bound %.3g" % (shape, name, worst))
        assert (np.abs(got - want) <= tol * mass).all(), (shape, name, worst)


def _parts(batch, channels, pixels):
    p, n = C.c_int(), C.c_int()
    assert _ffi.lib().rtod_bn_grad_parts(batch, channels, pixels, C.byref(p), C.byref(n)) == 0, _ffi.last_error()
    return p.value, n.value


def _rule(batch, channels, pixels):
    N = batch * pixels
    target = min(256, -(-2048 // channels))
    part_len = 1024 * -(-(-(-N // target)) // 1024)
    return -(-N // part_len), part_len


def test_partition_is_the_documented_rule_of_the_shape():
    B, C_, H, W = PARTS_SHAPE
    parts, part_len = _parts(B, C_, H * W)
    assert parts >= 3 and (B * H * W) % part_len != 0, (parts, part_len)          # several parts, a ragged tail
    shapes = [(b, c, h * w) for b, c, h, w in SHAPES] + [(8, 16, 416 * 416), (8, 1024, 13 * 13), (8, 64, 208 * 208), (1, 1, 1), (1, 4096, 7), (64, 1, 5000)]
    for s in shapes:
        parts, part_len = _parts(*s)
        assert (parts, part_len) == _rule(*s), s
        assert part_len % 1024 == 0 and (parts - 1) * part_len < s[0] * s[2] <= parts * part_len and parts <= 256, s
        nbytes = C.c_size_t()
        assert _ffi.lib().rtod_bn_grad_workspace(*s, C.byref(nbytes)) == 0 and nbytes.value == 16 * s[1] * parts, s
    # the largest layer gives every CU work, the deep layers keep four-wave workgroups with at least 1024 values each
    assert _parts(8, 16, 416 * 416) == (123, 11264) and _parts(8, 1024, 13 * 13) == (2, 1024)


def test_bn_grad_argument_checks():
    lib = _ffi.lib()
    p, n, nbytes = C.c_int(), C.c_int(), C.c_size_t()
    for shape in [(0, 1, 1), (1, 0, 1), (1, 1, 0), (1 << 15, 1, 1 << 14)]:
        assert lib.rtod_bn_grad_parts(*shape, C.byref(p), C.byref(n)) == -1 and "bn_grad_parts" in _ffi.last_error(), shape
        assert lib.rtod_bn_grad_workspace(*shape, C.byref(nbytes)) == -1 and "bn_grad_workspace" in _ffi.last_error(), shape
    assert lib.rtod_bn_grad_parts(1, 1, 1, None, C.byref(n)) == -1 and lib.rtod_bn_grad_workspace(1, 1, 1, None) == -1
    # the launcher refuses before anything is enqueued: fake, never dereferenced addresses
    ONE, ODD = C.c_void_p(4096), C.c_void_p(4100)
    call = lambda du=ONE, z=ONE, mean=ONE, var=ONE, gamma=ONE, shape=(1, 1, 1), dz=ONE, dg=ONE, db=ONE, ws=ONE, nb=16: \
        lib.rtod_bn_grad(du, z, mean, var, gamma, *shape, dz, dg, db, ws, nb, None)
    for kw in [dict(du=None), dict(z=None), dict(mean=None), dict(var=None), dict(gamma=None), dict(dz=None), dict(dg=None), dict(db=None), dict(ws=None),
               dict(shape=(0, 1, 1)), dict(shape=(1, 1, 0)), dict(du=ODD), dict(z=ODD), dict(dz=ODD), dict(ws=ODD), dict(mean=ODD), dict(nb=15),
               dict(shape=(1, 8, 67 * 61), nb=16 * 8 * 4 - 1)]:
        assert call(**kw) == -1, kw
        assert "bn_grad" in _ffi.last_error(), kw


# ---------------------------------------------------------------------------------------------- the plan option keep_bn_inputs
from head_grad_cases import describe, pack, plan  # noqa: E402
from realtimeobjectdetection_amd import cfgs, synth  # noqa: E402
from realtimeobjectdetection_amd.cfg import build_ir, parse_cfg_text  # noqa: E402
from scope_grad_cases import KEEP, plan_list  # noqa: E402

BATCH = [("bn_batch_stats", 1)]
KEPT = BATCH + [("keep_bn_inputs", 1)]
LISTINGS = [("rtod_plan_head_blocks", 3), ("rtod_plan_neck_layers", 2), ("rtod_plan_trainable_layers", 2), ("rtod_plan_full_layers", 2)]
CFGS = {"mini": cfgs.mini_cfg(64, 64), "pool_train_mini": cfgs.pool_train_mini_cfg(64, 64, stem=16)}
MAX_BATCH = 4


def _listings(h):
    return [plan_list(entry, h, columns) for entry, columns in LISTINGS]


@pytest.mark.parametrize("name", sorted(CFGS))
@pytest.mark.parametrize("scope", sorted(KEEP))
def test_listings_are_the_eval_plans_with_the_option_and_todays_without(name, scope):
    lib = _ffi.lib()
    keep = [(k, v) for k, v in KEEP[scope].items()]
    ev, on, off = plan(CFGS[name], 64, MAX_BATCH, 0, keep), plan(CFGS[name], 64, MAX_BATCH, 0, keep + KEPT), plan(CFGS[name], 64, MAX_BATCH, 0, keep + BATCH)
    want = _listings(ev)
    assert _listings(on) == want and any(len(rows) for rows in want[1:]), (name, scope)
    assert all(conv == -1 for _, conv, _ in _listings(off)[0]) and _listings(off)[1:] == [[], [], []]       # as today: nothing is trainable
    # the keep option keeps the same activations: every buffer of the eval plan has its twin, live over the same interval
    d_ev, d_on = describe(ev), describe(on)
    assert d_on["layers"] == d_ev["layers"] and d_on["bufs"][:len(d_ev["bufs"])] == [dict(b, offset=o["offset"]) for b, o in zip(d_ev["bufs"], d_on["bufs"])]
    for h in (ev, on, off):
        lib.rtod_plan_destroy(h)


def test_keep_bn_inputs_refusals():
    lib, err = _ffi.lib(), _ffi.last_error
    ONE = C.c_void_p(64)
    sgd = _ffi.OptStep(0, 1e-3, 0, 0, 0, 0)
    text = CFGS["mini"]
    keep = [(k, v) for k, v in KEEP["backbone"].items()]
    # a plan whose precision is not fp32, in either order of the two calls; the plan stays as it was
    h = plan(text, 64, MAX_BATCH, 1)
    before = describe(h)
    assert lib.rtod_plan_set_option(h, b"keep_bn_inputs", 1) == -3 and "keep_bn_inputs" in err() and describe(h) == before
    lib.rtod_plan_destroy(h)
    h = plan(text, 64, MAX_BATCH, 0, [("keep_bn_inputs", 1)])
    assert lib.rtod_plan_set_precision(h, 1) == -3 and "keep_bn_inputs" in err() and lib.rtod_plan_set_precision(h, 2) == -3
    lib.rtod_plan_destroy(h)
    on, ev = plan(text, 64, MAX_BATCH, 0, keep + KEPT), plan(text, 64, MAX_BATCH, 0, keep)
    layer = plan_list("rtod_plan_trainable_layers", ev, 2)[0][0]
    step_bn = lambda h, layer=layer: lib.rtod_plan_step_conv_bn(h, layer, C.byref(sgd), ONE, ONE, ONE, ONE, ONE, ONE, None, None, None, None, None, None, None)
    # the folded entries keep refusing a batch-statistics plan and name the new entry
    assert lib.rtod_plan_step_conv_folded(on, layer, C.byref(sgd), ONE, ONE, None, None, None) == -1 and "batch-statistics" in err() and "rtod_plan_step_conv_bn" in err()
    assert lib.rtod_plan_update_conv_weight(on, layer, ONE) == -1 and lib.rtod_plan_conv_scale(on, layer, None, None, 1) == -1 and "rtod_plan_step_conv_bn" in err()
    # ... and the new entries an eval plan, naming the folded one
    assert step_bn(ev) == -1 and "rtod_plan_step_conv_folded" in err()
    assert lib.rtod_plan_update_conv_bn(ev, layer, ONE, ONE, ONE) == -1 and lib.rtod_plan_read_bn_input(ev, layer, 1, ONE, None) == -1
    mean, var = C.c_void_p(), C.c_void_p()
    assert lib.rtod_plan_bn_stats_dev(ev, layer, C.byref(mean), C.byref(var)) == -1 and "bn_batch_stats" in err()
    # accepted convs get as far as the state check; the rest is refused with a reason, all before anything is enqueued
    assert step_bn(on) == -4 and "load_weights" in err() and lib.rtod_plan_read_bn_input(on, layer, 1, ONE, None) == -4
    assert lib.rtod_plan_bn_stats_dev(on, layer, C.byref(mean), C.byref(var)) == -4
    heads = [c for c, _, _ in plan_list("rtod_plan_head_blocks", on, 3)]
    assert step_bn(on, heads[0]) == -1 and "no BatchNorm" in err() and step_bn(on, 10 ** 6) == -1 and "not a convolution" in err()
    assert lib.rtod_plan_step_conv_bn(on, layer, None, ONE, ONE, ONE, ONE, ONE, ONE, None, None, None, None, None, None, None) == -1 and "null" in err()
    adam = _ffi.OptStep(1, 1e-3, 0.9, 0.999, 1e-8, 1)
    assert lib.rtod_plan_step_conv_bn(on, layer, C.byref(adam), ONE, ONE, ONE, ONE, ONE, ONE, ONE, ONE, ONE, ONE, ONE, None, None) == -1 and "moment" in err()
    no_option = plan(text, 64, MAX_BATCH, 0, keep + BATCH)
    assert step_bn(no_option) == -1 and "keep_bn_inputs" in err()
    # a conv with a shortcut added in its normalise step is no member of the narrower scopes, which do not hold that fusion
    neck = plan(text, 64, MAX_BATCH, 0, [(k, v) for k, v in KEEP["neck"].items()] + KEPT)
    fused = [L["index"] for L in describe(neck)["layers"] if L["type"] == "convolutional" and L["bn"] and L["fused_into"] >= 0 and
             describe(neck)["layers"][L["fused_into"]]["type"] == "shortcut"]
    assert fused and step_bn(neck, fused[0]) == -1 and "shortcut" in err() and "act(u)" in err()
    assert fused[0] not in [c for c, _ in plan_list("rtod_plan_neck_layers", neck, 2)]
    for h in (on, ev, no_option, neck):
        lib.rtod_plan_destroy(h)


@pytest.mark.parametrize("name,scope", [("mini", "blocks"), ("mini", "neck"), ("mini", "backbone"), ("pool_train_mini", "full")])
def test_arena_grows_by_the_kept_bn_inputs(name, scope):
    lib = _ffi.lib()
    keep = [(k, v) for k, v in KEEP[scope].items()]
    on, off = plan(CFGS[name], 64, MAX_BATCH, 0, keep + KEPT), plan(CFGS[name], 64, MAX_BATCH, 0, keep + BATCH)
    info_on, info_off = _ffi.PlanInfo(), _ffi.PlanInfo()
    assert lib.rtod_plan_get_info(on, C.byref(info_on)) == 0 and lib.rtod_plan_get_info(off, C.byref(info_off)) == 0
    entry, columns = {"blocks": LISTINGS[0], "neck": LISTINGS[1], "backbone": LISTINGS[2], "full": LISTINGS[3]}[scope]
    rows = plan_list(entry, on, columns)
    listed = [r[1] for r in rows if r[1] >= 0] if scope == "blocks" else [r[0] for r in rows]
    shape = {L.index: L.cout * L.hout * L.wout for L in build_ir(parse_cfg_text(CFGS[name]), 64).layers}
    assert listed and info_on.arena_bytes >= info_off.arena_bytes + 4 * MAX_BATCH * sum(shape[c] for c in listed), (name, scope)
    for h in (on, off):
        lib.rtod_plan_destroy(h)


def test_packed_image_does_not_depend_on_the_option_and_an_eval_plan_ignores_it():
    lib = _ffi.lib()
    text = CFGS["mini"]
    w = synth.synth_weights(build_ir(parse_cfg_text(text), 64))
    keep = [(k, v) for k, v in KEEP["backbone"].items()]
    on, off = plan(text, 64, MAX_BATCH, 0, keep + KEPT), plan(text, 64, MAX_BATCH, 0, keep + BATCH)
    assert np.array_equal(pack(on, w), pack(off, w))
    assert [dict(L) for L in describe(on)["layers"]] == describe(off)["layers"] and describe(on)["n_launches"] == describe(off)["n_launches"]
    # inert without bn_batch_stats: the same plan, the same image, the same arena
    inert, plain = plan(text, 64, MAX_BATCH, 0, keep + [("keep_bn_inputs", 1)]), plan(text, 64, MAX_BATCH, 0, keep)
    assert describe(inert) == describe(plain) and np.array_equal(pack(inert, w), pack(plain, w))
    for h in (on, off, inert, plain):
        lib.rtod_plan_destroy(h)
