"""Host tests (no GPU) of the split-f16 data gradient: rtod_conv_dgrad_split_tiles and _workspace through the C ABI, every refusal
of the three entries (all decided before anything touches the device), DarknetTrainer's grad_precision argument, and the float64
model of tests/dgrad_split_cases.py: against float64 truth it lies under the float32 floor, and the gate catches every planted
defect on every case it applies to."""
import ctypes as C
import types

import pytest
import torch

from dgrad_split_cases import GATE_M, GPU_CASES, HOST_CASES, HOST_IMAGE_RATIO, MUTANTS, applicable, floors, gate, make_inputs, model, record, residual, rms_max
from realtimeobjectdetection_amd import _ffi, cfgs
from realtimeobjectdetection_amd.cfg import parse_cfg_text
from realtimeobjectdetection_amd.train import DarknetTrainer, conv_dgrad_split_takes, conv_dgrad_split_tiles

# tile id ranges of the families (csrc/rtod_internal.h): generic 0-11; band 50-69, of which the bandd modes are 61-69 (K groups per
# mode: 1 1 1 2 2 1 2 - 2, mode 68 the wide tile); slab 90-100
TENSOR_SCALE_RATIO = 2.0 ** 24
GENERIC, BANDD_KG1, BANDD_KG2, WIDE, SLAB = set(range(12)), {61, 62, 63, 66}, {64, 65, 67, 69}, 68, set(range(90, 101))


def _workspace(*shape):
    n = C.c_size_t()
    assert _ffi.lib().rtod_conv_dgrad_split_workspace(*shape, C.byref(n)) == 0, _ffi.last_error()
    return n.value


def test_tiles_follow_the_forward_rules_without_a_device():
    got = {k: conv_dgrad_split_tiles(*s) for k, s in GPU_CASES.items()}
    assert set(got["A"]) == BANDD_KG1 and set(got["B"]) == BANDD_KG2                      # band layers: the bandd modes of their K-group count
    assert set(got["C"]) == GENERIC | {WIDE} and set(got["D"]) == GENERIC                  # 94 < W <= 160, Npad % 128 == 0: the wide tile too
    assert set(got["E"]) == GENERIC | SLAB and set(got["F"]) == GENERIC | SLAB             # 1x1, K a multiple of 64 (255 -> 256): the slab tiles too
    assert set(got["G"]) == GENERIC                                                         # K = 32
    for k, ids in got.items():
        assert len(ids) == len(set(ids)) and ids[1:] == sorted(ids[1:]), k                 # the default first, the rest ascending
    # a short buffer: the count, and as many ids as fit
    buf = (C.c_int * 2)()
    assert _ffi.lib().rtod_conv_dgrad_split_tiles(*GPU_CASES["D"], buf, 2) == 12 and list(buf) == got["D"][:2]
    # the batch moves the default of a generic layer only within its legal list
    assert set(conv_dgrad_split_tiles(64, 32, 32, 3, 168, 3)) == GENERIC


def test_workspace_holds_every_buffer_of_the_call():
    for shape in list(GPU_CASES.values()) + HOST_CASES + [(8, 1024, 512, 13, 13, 3), (8, 64, 32, 208, 208, 3)]:
        B, cout, cin, H, W, size = shape
        Kc, Npad, M, taps = -(-cout // 32) * 32, -(-cin // 128) * 128, B * H * W, size * size
        need = 4 * M * Kc + 2 * 2 * taps * Kc * Npad + 4 * M * Npad                          # split dz, two weight planes, the raw sums
        got = _workspace(*shape)
        assert need <= got <= need + 4 * (5 * Npad + 2 * B + 64 * B) + 8 * 16 * cin + 8 * 256, (shape, got, need)


def test_every_refusal_names_its_entry():
    lib = _ffi.lib()
    err = _ffi.last_error
    n, ids = C.c_size_t(), (C.c_int * 32)()
    bad_shapes = [(0, 64, 32, 13, 13, 3), (1, 0, 32, 13, 13, 3), (1, 64, 0, 13, 13, 3), (1, 64, 16, 13, 13, 3), (1, 64, 48, 13, 13, 3), (1, 64, 32, 0, 13, 3),
                  (1, 64, 32, 13, 0, 3), (1, 64, 32, 13, 13, 2), (1, 64, 32, 13, 13, 5), (65536, 64, 32, 1, 1, 1),
                  (8, 64, 32, 16384, 16384, 1),                                              # batch * pixels >= 2^31
                  (8, 1024, 32, 256, 256, 3),                                                # split dz: 4 * 524288 * 1024 bytes = 2 GiB
                  (1, 131072, 1024, 2, 2, 3)]                                                # weight plane: 2 * 9 * 131072 * 1024 bytes > 2 GiB
    ONE, ODD = C.c_void_p(4096), C.c_void_p(4100)
    call = lambda w=ONE, scale=None, dz=ONE, y=None, slope=0.1, shape=GPU_CASES["A"], tile=-1, dx=ONE, ws=ONE, nb=1 << 40: \
        lib.rtod_conv_dgrad_split(w, scale, dz, y, slope, *shape, tile, dx, ws, nb, None)
    for shape in bad_shapes:
        assert lib.rtod_conv_dgrad_split_tiles(*shape, ids, 32) == -1 and err().startswith("conv_dgrad_split_tiles:"), (shape, err())
        assert lib.rtod_conv_dgrad_split_workspace(*shape, C.byref(n)) == -1 and err().startswith("conv_dgrad_split_workspace:"), (shape, err())
        assert call(shape=shape) == -1 and err().startswith("conv_dgrad_split:"), (shape, err())
    assert "2 GiB" in (lib.rtod_conv_dgrad_split_workspace(8, 1024, 32, 256, 256, 3, C.byref(n)), err())[1]
    assert "2 GiB" in (lib.rtod_conv_dgrad_split_workspace(1, 131072, 1024, 2, 2, 3, C.byref(n)), err())[1]
    assert lib.rtod_conv_dgrad_split_workspace(8, 1024, 32, 256, 255, 3, C.byref(n)) == 0      # just below the limit
    assert lib.rtod_conv_dgrad_split_tiles(*GPU_CASES["A"], None, 4) == -1 and err().startswith("conv_dgrad_split_tiles:")
    assert lib.rtod_conv_dgrad_split_workspace(*GPU_CASES["A"], None) == -1 and err().startswith("conv_dgrad_split_workspace:")
    # the launcher refuses before anything is enqueued: fake, never dereferenced addresses
    need = _workspace(*GPU_CASES["A"])
    legal = conv_dgrad_split_tiles(*GPU_CASES["A"])
    illegal = [t for t in (-2, 0, 5, 50, 64, 68, 70, 90, 110, 140, 150, 1000) if t not in legal]
    for kw in [dict(w=None), dict(dz=None), dict(dx=None), dict(ws=None), dict(nb=need - 1), dict(nb=0), dict(ws=ODD), dict(slope=float("nan")),
               dict(w=C.c_void_p(4098)), dict(dz=C.c_void_p(4097)), dict(dx=C.c_void_p(4099)), dict(y=C.c_void_p(4097)), dict(scale=ODD)] + [dict(tile=t) for t in illegal]:
        assert call(**kw) == -1 and err().startswith("conv_dgrad_split:"), (kw, err())
    assert "not a legal tile" in (call(tile=0), err())[1] and "workspace has" in (call(nb=need - 1), err())[1]


def test_grad_precision_is_validated_and_defaults_to_fp32():
    stub = lambda: types.SimpleNamespace(blocks=parse_cfg_text(cfgs.mini_cfg(64, 64)), net_info={"height": 64}, input_width=None, options={})
    assert DarknetTrainer(stub()).grad_precision == "fp32"
    assert DarknetTrainer(stub(), grad_precision="f16s3").grad_precision == "f16s3"
    for bad in ("f16", "fp16", "FP32", None, 1, ""):
        with pytest.raises(ValueError, match="grad_precision"):
            DarknetTrainer(stub(), grad_precision=bad)
    # what the walk sends to the split entry: stride 1, size 1 or 3, Cin a positive multiple of 32
    assert conv_dgrad_split_takes(32, 1) and conv_dgrad_split_takes(512, 3) and conv_dgrad_split_takes(64, 3, 1)
    assert not any(conv_dgrad_split_takes(*a) for a in [(16, 3), (3, 3), (48, 1), (64, 3, 2), (64, 5), (0, 1)])


_records = {}


def _case(case, ratio=HOST_IMAGE_RATIO):
    """Inputs and record of a host case, computed once and shared (never modified)."""
    if (case, ratio) not in _records:
        w, scale, dz, y = make_inputs(case, ratio)
        with torch.no_grad():
            _records[case, ratio] = ((w, scale, dz, y), record(w, scale, dz, y, case[5]))
    return _records[case, ratio]


@pytest.mark.parametrize("case", HOST_CASES, ids=lambda c: "x".join(map(str, c)))
def test_the_format_lies_under_the_float32_floor_and_the_gate_catches_every_mutant(case):
    """Against the float64 transposed conv of the same operands, in units of D = conv_T(|dz|, |v|): the model's rms and max error are at
    most those of torch's float32 conv_transpose2d (the larger of NCHW and channels_last) — the format costs nothing against float32
    (measured on the CPU: 0.04 - 0.27 of that floor).  Then the teeth: the float32 references pass the 4 x gate against the model, and
    each mutant of dgrad_split_cases.MUTANTS fails it.

    tensor_scale is judged on the same shapes with the images 2^24 apart (TENSOR_SCALE_RATIO).  At 1000 x a scale per tensor costs
    the smaller image 10 of the 13 bits of headroom between the planes' range (2^13) and the hi plane's normal range (2^-14): every
    element that carries weight in D still has its 22 bits, and the defect measures 0.2 - 0.3 of the float32 floor (512/64: rms 0.3 x,
    max 0.2 x) — below ANY gate built on that floor, so those inputs give the gate no teeth against it.  At 2^24 the smaller image
    falls into the f16 subnormals under a tensor-wide scale and stays exact under its own; the bit-for-bit batch independence of
    tests/test_dgrad_split_gpu.py holds the per-image scale at every ratio."""
    (w, scale, dz, y), rec = _case(case)
    size = case[5]
    f_rms, f_max = floors(rec, "truth", ("nchw", "channels_last"))
    rms, mx = rms_max(residual(rec["model"], rec, "truth"))
    print("%s: model vs float64 truth rms/D %.3g max/D %.3g; float32 floor %.3g / %.3g; ratios %.2f / %.2f" % (case, rms, mx, f_rms, f_max, rms / f_rms, mx / f_max))
    for k, v in rec["refs"].items():
        print("    float32 %-14s vs model rms/D %.3g max/D %.3g" % ((k,) + rms_max(residual(v, rec))))
    assert rms <= f_rms and mx <= f_max, (case, rms / f_rms, mx / f_max)
    fl = floors(rec)
    for k, v in rec["refs"].items():
        assert gate(residual(v, rec), fl)[0], k
    passed = []
    for mutant in MUTANTS:
        if not applicable(mutant, case):
            continue
        (mw, mscale, mdz, my), mrec = _case(case, TENSOR_SCALE_RATIO) if mutant == "tensor_scale" else _case(case)
        mfl = floors(mrec)
        with torch.no_grad():
            r = residual(model(mw, mscale, mdz, my, size, mutant=mutant), mrec)
        ok, q_rms, q_max = gate(r, mfl)
        print("    mutant %-18s rms/D %.3g (%.1f x F_rms)  max/D %.3g (%.1f x F_max)%s" % ((mutant,) + (rms_max(r)[0], q_rms, rms_max(r)[1], q_max) + ("   PASSES THE GATE" if ok else "",)))
        if ok:
            passed.append(mutant)
    assert not passed, "the gate (m = %g) is too loose for %s: %s" % (GATE_M, case, passed)
