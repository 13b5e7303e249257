"""GPU tests of rtod_conv_dgrad_split (csrc/dgrad_split.hip): the data gradient of a stride-1 1x1 / 3x3 conv on the forward's
split-f16 MFMA tiles, held to the float64 model of tests/dgrad_split_cases.py and to the properties the entry promises.

Cases (dgrad_split_cases.GPU_CASES; B, Cout, Cin, H, W, size): A band layer with one K group (M = 338 leaves a tail in every tile), B
band layer with two K groups, C the wide tile, D generic tiles only, E slab tiles, F ragged K (Cout 255), G a generic 1x1.  dz is
heavy-tailed with the images of a batch 2^10 apart; y has positives, negatives and exact zeros; every case runs with and without a
row scale.

The gate is the forward's (tests/f16s3_emulation.py): r = (dx - model) / D with D = conv_T(|dz|, |v|); rms(r) and max|r| at most
GATE_M = 4 x the same figures of the float32 references (torch conv_transpose2d on NCHW and channels_last, and the float32
accumulation of the three products in the kernels' K order), all computed on the CPU from the same operands."""
import numpy as np
import pytest
import torch

from dgrad_split_cases import GATE_M, GPU_CASES, GPU_IMAGE_RATIO, SLOPE, floors, gate, make_inputs, record, residual, rms_max
from realtimeobjectdetection_amd import train as T

pytestmark = pytest.mark.gpu
NAMES = sorted(GPU_CASES)
BOTH = [False, True]

_cache = {}


def _setup(name, scaled):
    """Inputs (CPU and device), the CPU record and the default tile's dx of a case: computed once, shared, never modified."""
    key = (name, scaled)
    if key not in _cache:
        case = GPU_CASES[name]
        w, scale, dz, y = make_inputs(case, GPU_IMAGE_RATIO, seed=1, scaled=scaled)
        with torch.no_grad():
            rec = record(w, scale, dz, y, case[5])
        dev = tuple(None if t is None else t.cuda() for t in (w, scale, dz, y))
        _cache[key] = {"case": case, "cpu": (w, scale, dz, y), "dev": dev, "rec": rec, "floors": floors(rec), "dx": _run(dev, case[5])}
    return _cache[key]


def _run(dev, size, y=True, slope=SLOPE, tile=None, dz=None):
    w, scale, dz0, y0 = dev
    return T.conv_dgrad_split_async(w, dz0 if dz is None else dz, size, scale, y0 if y is True else y, slope, tile)


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_the_cases_reach_every_family():
    """Between them the legal lists hold a bandd tile of each K-group count, the wide tile, a slab tile and a generic tile."""
    ids = {k: set(T.conv_dgrad_split_tiles(*s)) for k, s in GPU_CASES.items()}
    every = set().union(*ids.values())
    assert every & {61, 62, 63, 66} and every & {64, 65, 67, 69} and 68 in every and every & set(range(90, 101)) and every & set(range(12)), ids
    assert ids["A"] <= {61, 62, 63, 66} and ids["B"] <= {64, 65, 67, 69} and 68 in ids["C"] and ids["D"] <= set(range(12)) and ids["E"] & set(range(90, 101))


@pytest.mark.parametrize("scaled", BOTH)
@pytest.mark.parametrize("name", NAMES)
def test_every_legal_tile_gives_the_same_bits_inside_the_gate(name, scaled):
    s = _setup(name, scaled)
    case, size = s["case"], s["case"][5]
    ok, q_rms, q_max = gate(residual(s["dx"].cpu(), s["rec"]), s["floors"])
    print("%s %s%s: default tile rms %.2f x F_rms, max %.2f x F_max (floors %.3g / %.3g)" % ((name, case, " scaled" if scaled else "", q_rms, q_max) + s["floors"]))
    assert ok and tuple(s["dx"].shape) == (case[0], case[2], case[3], case[4]), (name, scaled, q_rms, q_max, GATE_M)
    tiles = T.conv_dgrad_split_tiles(*case)
    for tile in tiles:
        assert _same(_run(s["dev"], size, tile=tile), s["dx"]), (name, scaled, tile)
    assert _same(_run(s["dev"], size), s["dx"]) and _same(_run(s["dev"], size, tile=tiles[-1]), s["dx"])      # repeatable from call to call


@pytest.mark.parametrize("scaled", BOTH)
@pytest.mark.parametrize("name", NAMES)
def test_an_image_does_not_depend_on_its_batch_and_scales_exactly(name, scaled):
    s = _setup(name, scaled)
    size = s["case"][5]
    w, scale, dz, y = s["dev"]
    for b in range(s["case"][0]):                                     # each image alone gives the bits it has inside the batch
        alone = T.conv_dgrad_split_async(w, dz[b:b + 1], size, scale, y[b:b + 1], SLOPE)
        assert _same(alone, s["dx"][b:b + 1]), (name, scaled, b)
    # the mask: one multiplication of the unmasked result
    plain = _run(s["dev"], size, y=None, slope=1.0)
    m = torch.where(y > 0, torch.ones_like(y), torch.full_like(y, SLOPE))
    assert _same(plain * m, s["dx"]) and _same(_run(s["dev"], size, slope=1.0), plain) and _same(_run(s["dev"], size, y=None), plain), (name, scaled)
    # dz 2^-20 gives dx 2^-20, bit for bit
    assert _same(_run(s["dev"], size, dz=dz * 2.0 ** -20), s["dx"] * 2.0 ** -20), (name, scaled)
    # an all-zero image gives exact zeros and leaves the other image as it was
    if s["case"][0] >= 2:
        dz0 = dz.clone()
        dz0[1] = 0.0
        got = _run(s["dev"], size, dz=dz0)
        assert not got[1].any() and _same(got[0], s["dx"][0]), (name, scaled)


@pytest.mark.parametrize("scaled", BOTH)
def test_ragged_k_padding_of_the_workspace_never_reaches_dx(scaled):
    """Case F (Cout 255: K padded to 256 with a zero channel).  Every byte of the cached workspace is set to 0xFF — NaN as a float, a
    half or a double — before the call; the result is finite and holds the bits of the first call."""
    s = _setup("F", scaled)
    case = s["case"]
    key = T._ffi.stream_key(s["dx"].device) + ("rtod_conv_dgrad_split", case)
    assert key in T._ffi.cache, "the workspace of case F is cached per shape"
    ws = [T._ffi.workspace("rtod_conv_dgrad_split", s["dx"].device, *case)[0]]
    for tile in T.conv_dgrad_split_tiles(*case)[:3]:
        for t in ws:
            t.fill_(0xFF)
        got = _run(s["dev"], case[5], tile=tile)
        assert bool(torch.isfinite(got).all()) and _same(got, s["dx"]), (scaled, tile)


def test_tensor_checks_of_the_python_entry():
    s = _setup("G", False)
    w, scale, dz, y = s["dev"]
    with pytest.raises(ValueError, match="conv_dgrad_split"):
        T.conv_dgrad_split_async(w, dz[:, :16], 1)
    with pytest.raises(ValueError, match="conv_dgrad_split"):
        T.conv_dgrad_split_async(w, dz, 1, y=y[:, :, :2])
    with pytest.raises(T._ffi.RtodError, match="not a legal tile"):
        T.conv_dgrad_split_async(w, dz, 1, tile=61)
    assert np.isfinite(rms_max(residual(s["dx"].cpu(), s["rec"]))).all()
