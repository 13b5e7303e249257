"""Host tests (no GPU) of the split-f16 weight gradient: the float64 model of tests/wgrad_split_cases.py (inside the gate against
float64 truth; the gate catches every planted defect on every case it applies to), rtod_conv_wgrad_split_schedule, _workspace and
_bounds through the C ABI, every refusal of the entries (all decided before anything touches the device), and DarknetTrainer's
wgrad_precision argument."""
import ctypes as C
import types

import pytest
import torch

from wgrad_split_cases import CASES, F_PADDING_ZEROS, GATE_M, MUTANTS, applicable, floors, gate, make_inputs, model, record, residual, rms_max
from realtimeobjectdetection_amd import _ffi, cfgs
from realtimeobjectdetection_amd import train as T
from realtimeobjectdetection_amd.cfg import parse_cfg_text

# the cases, YOLOv3's stride-1 shapes at 416x416 batch 8 (the largest and the smallest map, 1x1 and 3x3), a large tile grid and odd sizes
SWEEP = list(CASES.values()) + [(8, 64, 32, 208, 208, 3), (8, 32, 64, 208, 208, 1), (8, 1024, 512, 13, 13, 3), (8, 512, 1024, 13, 13, 1), (8, 256, 128, 52, 52, 3),
                                (1, 2048, 2048, 2, 2, 3), (1, 1, 32, 1, 1, 1), (1, 1, 32, 1, 1, 3), (5, 33, 96, 7, 31, 3), (4, 255, 256, 26, 26, 1), (7, 70, 32, 3, 5, 1)]


def _schedule(*shape):
    return T.conv_wgrad_split_schedule(*shape)


def _workspace(*shape):
    n = C.c_size_t()
    assert _ffi.lib().rtod_conv_wgrad_split_workspace(*shape, C.byref(n)) == 0, _ffi.last_error()
    return n.value


def _bounds(*shape):
    lo, hi, n = C.c_int64(), C.c_int64(), C.c_int64()
    assert _ffi.lib().rtod_conv_wgrad_split_bounds(*shape, C.byref(lo), C.byref(hi), C.byref(n)) == 0, _ffi.last_error()
    return lo.value, hi.value, n.value


def test_schedule_is_a_function_of_the_shape_over_the_padded_k():
    seen = set()
    for shape in SWEEP:
        B, cout, cin, H, W, size = shape
        tiles, slices, slice_len, kp = _schedule(*shape)
        grid = B * (H + 2) * (-(-(W + 2) // 8) * 8) if size == 3 else B * H * W
        tile = 64 if size == 3 else 128                               # 64 filters x 64 channels x nine taps, or 128 x 128
        assert kp % 8 == 0 and kp % 16 == 0 and grid <= kp < grid + 16, (shape, kp)
        assert tiles == -(-cout // tile) * -(-cin // tile) and 1 <= slices <= 64 and slice_len % 16 == 0, (shape, tiles, slices, slice_len)
        assert (slices - 1) * slice_len < kp <= slices * slice_len, (shape, slices, slice_len, kp)
        assert slices == 1 or slice_len >= 64, shape                  # no slivers
        assert _schedule(*shape) == (tiles, slices, slice_len, kp)
        seen |= {"one slice"} if slices == 1 else {"several slices"}
        seen |= {"several tiles"} if tiles > 1 else set()
    assert seen == {"one slice", "several slices", "several tiles"}
    assert _schedule(*CASES["G"])[1] > 1 and _schedule(*CASES["E"])[0] > 1 and _schedule(1, 2048, 2048, 2, 2, 3)[:2] == (1024, 1)


def test_workspace_grows_with_every_argument():
    """Any larger batch, height or width never shrinks the workspace.  In cout and cin the statement is for doubling: a larger tile grid
    takes fewer slices (at most half as many for twice the tiles), so one more tile may shrink the slice-sum buffer by more than the
    planes grow, while twice the channels hold twice the elements per slice."""
    for shape in SWEEP:
        B, cout, cin, H, W, size = shape
        base = _workspace(*shape)
        planes = 2 * 2 * (cout + cin) * _schedule(*shape)[3]          # hi and lo, two bytes, without the guards
        assert base >= planes + 4 * cout * cin * size * size * _schedule(*shape)[1], shape
        for bigger in [(B + 1, cout, cin, H, W, size), (B, cout, cin, H + 1, W, size), (B, cout, cin, H, W + 1, size), (B, cout, cin, H + 3, W + 9, size),
                       (B, 2 * cout, cin, H, W, size), (B, cout, 2 * cin, H, W, size)]:
            assert _workspace(*bigger) >= base, (shape, bigger)


def test_the_gemm_reads_only_halves_the_split_writes():
    """rtod_conv_wgrad_split_bounds: the lowest and the highest half index the GEMM forms for a shape (front guard at tap (0, 0) with the
    dword before it; the last step of the last slice at tap (2, 2) with the dword behind it), from the start of a plane.  The split
    kernel writes every half of every plane, so both inside [0, plane) is the bounds check of the call; a GPU sanitizer is not
    available for it."""
    for shape in SWEEP:
        B, cout, cin, H, W, size = shape
        lo, hi, plane = _bounds(*shape)
        tiles, slices, slice_len, kp = _schedule(*shape)
        assert 0 <= lo <= hi < plane and plane % 8 == 0, (shape, lo, hi, plane)
        if size == 3:
            wp = -(-(W + 2) // 8) * 8
            assert plane == kp + 2 * (wp + 8) and lo == 6 and hi == (wp + 8) + kp + wp + 1, (shape, lo, hi, plane)
        else:
            assert plane == kp and lo == 0 and hi == kp - 1, (shape, lo, hi, plane)


def test_every_refusal_names_its_entry():
    lib, err = _ffi.lib(), _ffi.last_error
    n, i4, i8 = C.c_size_t(), [C.c_int() for _ in range(3)], [C.c_int64() for _ in range(3)]
    ONE, ODD = C.c_void_p(4096), C.c_void_p(4100)
    call = lambda dz=ONE, x=ONE, shape=CASES["A"], scale=None, dw=ONE, ws=ONE, nb=1 << 40: lib.rtod_conv_wgrad_split(dz, x, *shape, scale, dw, ws, nb, None)
    bad_shapes = [(0, 64, 32, 13, 13, 3), (1, 0, 32, 13, 13, 3), (1, 64, 0, 13, 13, 3), (1, 64, 16, 13, 13, 3), (1, 64, 48, 13, 13, 1), (1, 64, 32, 0, 13, 3),
                  (1, 64, 32, 13, 0, 3), (1, 64, 32, 13, 13, 2), (1, 64, 32, 13, 13, 5),
                  (8, 32, 32, 16384, 8192, 1),                          # a plane of 2^30 halves: 2 GiB
                  (8, 32, 32, 16384, 16384, 1), (8, 32, 32, 16384, 16384, 3),    # the k grid beyond int32
                  (1, 65536, 65536, 2, 2, 1),                           # cout * cin beyond int32
                  (1, 65504, 32, 2, 2, 1)]                              # cout + cin rows beyond the split kernel's grid
    for shape in bad_shapes:
        assert lib.rtod_conv_wgrad_split_schedule(*shape, *(C.byref(v) for v in i4), C.byref(i8[0])) == -1 and err().startswith("conv_wgrad_split_schedule:"), (shape, err())
        assert lib.rtod_conv_wgrad_split_workspace(*shape, C.byref(n)) == -1 and err().startswith("conv_wgrad_split_workspace:"), (shape, err())
        assert lib.rtod_conv_wgrad_split_bounds(*shape, *(C.byref(v) for v in i8)) == -1 and err().startswith("conv_wgrad_split_bounds:"), (shape, err())
        assert call(shape=shape) == -1 and err().startswith("conv_wgrad_split:"), (shape, err())
    assert "2 GiB" in (lib.rtod_conv_wgrad_split_workspace(8, 32, 32, 16384, 8192, 1, C.byref(n)), err())[1]
    assert lib.rtod_conv_wgrad_split_workspace(8, 32, 32, 16384, 8191, 1, C.byref(n)) == 0, err()      # just below the limit
    assert lib.rtod_conv_wgrad_split_workspace(*CASES["A"], None) == -1 and err().startswith("conv_wgrad_split_workspace:")
    assert lib.rtod_conv_wgrad_split_schedule(*CASES["A"], None, None, None, None) == -1 and err().startswith("conv_wgrad_split_schedule:")
    assert lib.rtod_conv_wgrad_split_bounds(*CASES["A"], None, None, None) == -1 and err().startswith("conv_wgrad_split_bounds:")
    # the launcher refuses before anything is enqueued: fake, never dereferenced addresses
    need = _workspace(*CASES["A"])
    for kw in [dict(dz=None), dict(x=None), dict(dw=None), dict(ws=None), dict(nb=need - 1), dict(nb=0), dict(ws=ODD), dict(dz=C.c_void_p(4097)),
               dict(x=C.c_void_p(4098)), dict(dw=C.c_void_p(4099)), dict(scale=ODD)]:
        assert call(**kw) == -1 and err().startswith("conv_wgrad_split:"), (kw, err())
    assert "workspace has" in (call(nb=need - 1), err())[1]
    for phases in (0, -1, 16, 100):
        assert lib.rtod_conv_wgrad_split_phases(ONE, ONE, *CASES["A"], None, ONE, ONE, 1 << 40, None, phases) == -1 and "phases" in err()


def test_wgrad_precision_is_validated_and_defaults_to_fp32():
    stub = lambda: types.SimpleNamespace(blocks=parse_cfg_text(cfgs.mini_cfg(64, 64)), net_info={"height": 64}, input_width=None, options={})
    t = T.DarknetTrainer(stub())
    assert t.wgrad_precision == "fp32" and t.grad_precision == "fp32"
    t = T.DarknetTrainer(stub(), wgrad_precision="f16s3")
    assert t.wgrad_precision == "f16s3" and t.grad_precision == "fp32"            # the two arguments are independent
    t = T.DarknetTrainer(stub(), grad_precision="f16s3")
    assert t.wgrad_precision == "fp32" and t.grad_precision == "f16s3"
    for bad in ("f16", "fp16", "FP32", None, 1, ""):
        with pytest.raises(ValueError, match="wgrad_precision"):
            T.DarknetTrainer(stub(), wgrad_precision=bad)
    assert set(T.WGRAD_SPLIT_SIZES) <= {1, 3}
    assert T.conv_wgrad_split_takes(32, 1) and T.conv_wgrad_split_takes(512, 3) and T.conv_wgrad_split_takes(64, 3, 1)
    assert not any(T.conv_wgrad_split_takes(*a) for a in [(16, 3), (3, 3), (48, 1), (64, 3, 2), (64, 5), (0, 1)])


_records = {}


def _case(name, scaled):
    """Inputs and record of a case, computed once and shared (never modified)."""
    if (name, scaled) not in _records:
        dz, x, scale = make_inputs(CASES[name], scaled=scaled)
        with torch.no_grad():
            _records[name, scaled] = ((dz, x, scale), record(dz, x, scale, CASES[name][5]))
    return _records[name, scaled]


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_model_is_inside_the_gate_and_the_gate_catches_every_mutant(name):
    """Against the float64 weight gradient of the same operands, in units of D: the model's rms and max error are inside the gate built
    on the float32 references' own error against that truth (measured on the CPU: the format's rms error is 0.14 - 0.80 of that floor).
    Then the teeth: the float32 references pass the 4 x gate against the model, and each applicable mutant of wgrad_split_cases.MUTANTS
    fails it.  Case F: the 6144 elements of dW whose every term is padding are exact zeros in the model."""
    case = CASES[name]
    (dz, x, scale), rec = _case(name, True)
    size = case[5]
    t_floor = floors(rec, "truth")
    ok, q_rms, q_max = gate(residual(rec["model"], rec, "truth"), t_floor)
    print("%s %s: model vs float64 truth %.2f x F_rms, %.2f x F_max (floors %.3g / %.3g)" % ((name, case, q_rms, q_max) + t_floor))
    assert ok, (name, q_rms, q_max)
    fl = floors(rec)
    for k, v in rec["refs"].items():
        print("    float32 %-14s vs model rms/D %.3g max/D %.3g" % ((k,) + rms_max(residual(v, rec))))
        assert gate(residual(v, rec), fl)[0], k
    if name == "F":
        assert int(rec["zero"].sum()) == F_PADDING_ZEROS and not rec["model"][rec["zero"]].any()
    passed, tried = [], []
    for mutant in MUTANTS:
        if not applicable(mutant, case):
            continue
        tried.append(mutant)
        with torch.no_grad():
            r = residual(model(dz, x, scale, size, mutant=mutant), rec)
        ok, q_rms, q_max = gate(r, fl)
        print("    mutant %-16s %.3g x F_rms  %.3g x F_max%s" % (mutant, q_rms, q_max, "   PASSES THE GATE" if ok else ""))
        if ok:
            passed.append(mutant)
    assert tried and not passed, "the gate (m = %g) is too loose for %s: %s" % (GATE_M, case, passed)


def test_every_mutant_applies_to_some_case():
    assert all(any(applicable(m, c) for c in CASES.values()) for m in MUTANTS)
