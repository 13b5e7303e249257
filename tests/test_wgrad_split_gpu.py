"""GPU tests of rtod_conv_wgrad_split (csrc/wgrad_split.hip): the weight gradient of a stride-1 1x1 / 3x3 conv as three f16 MFMA
products, held to the float64 model of tests/wgrad_split_cases.py and to the properties the entry promises.

Cases (wgrad_split_cases.CASES; B, Cout, Cin, H, W, size): A odd width, B a map smaller than a k step's row group, C W % 8 == 0 and a
Cout tile tail, D a ragged 1x1 with K % 8 != 0, E a Cin column tail over several tiles, F one row (six of nine taps see only
padding), G several K slices.  dz is heavy-tailed with the images of a batch 2^10 apart, x is leaky-shaped with exact zeros; every
case runs with and without a row scale.

The gate is the forward's (tests/f16s3_emulation.py): r = (dW - model) / D with D = |row_scale| conv2d_weight(|x|, |dz|); rms(r) and
max|r| at most GATE_M = 4 x the same figures of the float32 references (torch conv2d_weight on NCHW and channels_last, and the float32
accumulation of the three products), all computed on the CPU from the same operands.

Measured on an MI355X over the seven cases, with and without a row scale: rms 0.27 - 0.83 x F_rms, max 0.19 - 0.73 x F_max."""
import pytest
import torch

from wgrad_split_cases import CASES, F_PADDING_ZEROS, GATE_M, floors, gate, make_inputs, record, residual
from realtimeobjectdetection_amd import train as T

pytestmark = pytest.mark.gpu
NAMES = sorted(CASES)
BOTH = [False, True]

_cache = {}


def _setup(name, scaled):
    """Inputs (CPU and device), the CPU record and the first call's dW of a case: computed once, shared, never modified."""
    key = (name, scaled)
    if key not in _cache:
        case = CASES[name]
        dz, x, scale = make_inputs(case, scaled=scaled)
        with torch.no_grad():
            rec = record(dz, x, scale, case[5])
        dev = tuple(None if t is None else t.cuda() for t in (dz, x, scale))
        _cache[key] = {"case": case, "dev": dev, "rec": rec, "floors": floors(rec), "dw": T.conv_wgrad_split_async(dev[0], dev[1], case[5], dev[2])}
    return _cache[key]


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("scaled", BOTH)
@pytest.mark.parametrize("name", NAMES)
def test_dw_is_inside_the_gate_and_repeats_bit_for_bit(name, scaled):
    s = _setup(name, scaled)
    case, size = s["case"], s["case"][5]
    dz, x, scale = s["dev"]
    ok, q_rms, q_max = gate(residual(s["dw"].cpu(), s["rec"]), s["floors"])
    print("%s %s%s: rms %.2f x F_rms, max %.2f x F_max (floors %.3g / %.3g), schedule %s" % ((name, case, " scaled" if scaled else "", q_rms, q_max) + s["floors"] + (T.conv_wgrad_split_schedule(*case),)))
    assert tuple(s["dw"].shape) == (case[1], case[2], size, size)
    assert ok, (name, scaled, q_rms, q_max, GATE_M)
    assert _same(T.conv_wgrad_split_async(dz, x, size, scale), s["dw"])                          # repeatable from call to call
    assert _same(T.conv_wgrad_split_async(dz, x, size, scale, phases=15), s["dw"])               # the measurement entry's full call
    exact = T.conv_wgrad_async(dz, x, size, row_scale=scale)[0]
    assert not _same(exact, s["dw"]), "the split entry gave the exact entry's bits: is it on the path?"


@pytest.mark.parametrize("scaled", BOTH)
@pytest.mark.parametrize("name", NAMES)
def test_powers_of_two_and_zeros_pass_through_exactly(name, scaled):
    s = _setup(name, scaled)
    size = s["case"][5]
    dz, x, scale = s["dev"]
    assert _same(T.conv_wgrad_split_async(dz * 2.0 ** -20, x, size, scale), s["dw"] * 2.0 ** -20), (name, scaled)
    assert _same(T.conv_wgrad_split_async(dz, x * 2.0 ** 7, size, scale), s["dw"] * 2.0 ** 7), (name, scaled)
    assert not T.conv_wgrad_split_async(torch.zeros_like(dz), x, size, scale).any(), (name, scaled)
    if name == "F":                                                   # the taps that see only padding
        zero = s["rec"]["zero"].cuda()
        assert int(zero.sum()) == F_PADDING_ZEROS and not s["dw"][zero].any() and bool(s["dw"][~zero].any())


@pytest.mark.parametrize("scaled", BOTH)
@pytest.mark.parametrize("name", ["A", "D", "F"])
def test_nothing_the_call_did_not_write_reaches_dw(name, scaled):
    """Every byte of the cached workspace is set to 0xFF — NaN as a float, a half or a double — before the call; the result is finite
    and holds the bits of the first call: guards, halo, the tail of the k grid and the slice sums are all written by the call itself."""
    s = _setup(name, scaled)
    case = s["case"]
    dz, x, scale = s["dev"]
    key = T._ffi.stream_key(dz.device) + ("rtod_conv_wgrad_split", case)
    assert key in T._ffi.cache, "the workspace of the case is cached per shape"
    T._ffi.workspace("rtod_conv_wgrad_split", dz.device, *case)[0].fill_(0xFF)
    got = T.conv_wgrad_split_async(dz, x, case[5], scale)
    assert bool(torch.isfinite(got).all()) and _same(got, s["dw"]), (name, scaled)


def test_tensor_checks_of_the_python_entry():
    s = _setup("B", False)
    dz, x, _ = s["dev"]
    launched = len(T._ffi.cache)
    with pytest.raises(ValueError, match="conv_wgrad_split"):
        T.conv_wgrad_split_async(dz, x[:, :, :2], 3)                  # maps differ
    with pytest.raises(ValueError, match="conv_wgrad_split"):
        T.conv_wgrad_split_async(dz, x.double(), 3)
    with pytest.raises(ValueError, match="row_scale"):
        T.conv_wgrad_split_async(dz, x, 3, row_scale=torch.ones(5, dtype=torch.float64, device=dz.device))
    with pytest.raises(T._ffi.RtodError, match="conv_wgrad_split"):
        T.conv_wgrad_split_async(dz, x[:, :16].contiguous(), 3)       # Cin 16: refused by the library, before any launch
    with pytest.raises(T._ffi.RtodError, match="conv_wgrad_split"):
        T.conv_wgrad_split_async(dz, x, 5)
    assert len(T._ffi.cache) == launched                              # no workspace was made for a refused shape
    assert _same(T.conv_wgrad_split_async(dz, x, 3), s["dw"])
