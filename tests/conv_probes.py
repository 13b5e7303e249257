"""Probe networks for the split-f16 / plain-f16 conv tiles (test helper; tests/test_f16s3_emulation_host.py and
tests/test_f16s3_local_gpu.py).

Whole networks only reach the layer shapes their input sizes produce (widths 8 ... 304 of a few kinds, input channels powers
of two plus some concat sums).  Plan::tile_legal admits much more.  A probe is the smallest graph that puts ONE convolution of a
chosen shape (H, W, Cin, Cout, k, stride, activation, with or without a fused shortcut) into a plan:

    stem 3x3 (3 -> 32)  [16 filters under narrow_cin]
    optionally 1x1 (32 -> Cin)
    the conv under test
    optionally [shortcut] (the 1x1 then produces Cin = Cout channels and the shortcut reads it)
    1x1 linear head with 24 filters + [yolo] with 3 classes (grid = the map: stride 1, or 2 below a stride-2 conv)

PROBES lists them with what each one reaches; ``legal_ids`` enumerates, through the C ABI alone (no device), the tile ids
rtod_plan_set_tiles accepts for the conv under test.
"""
import ctypes as C
from dataclasses import dataclass, field

from realtimeobjectdetection_amd import _ffi
from realtimeobjectdetection_amd.cfgs import _ANCHORS_V3, _conv, _net, _shortcut, _yolo

CLASSES = 3
IDS = range(170)
# every id of every split-f16 tile family (csrc/split_tiles.cpp): generic, band (LDS 50-56 / 61-63 / 66, two-K-group 57-60 / 64 / 65 /
# 67 / 69, wide bandd 68), ring, 1x1 slab, patch, narrow, K-sliced
FAMILIES = {"generic": range(0, 12), "band": range(50, 70), "ring": range(70, 78), "slab": range(90, 101),
            "patch": range(110, 115), "narrow": range(140, 144), "ksliced": range(150, 156)}


@dataclass(frozen=True)
class Probe:
    name: str
    H: int
    W: int
    cin: int
    cout: int
    k: int
    stride: int
    B: int
    act: str = "leaky"
    shortcut: bool = False
    options: tuple = ()                      # ((name, value), ...) of rtod_plan_set_option
    note: str = field(default="", compare=False)

    @property
    def stem(self):
        return 16 if self.cin == 16 else 32

    @property
    def has_1x1(self):
        return self.cin != self.stem or self.shortcut

    @property
    def conv_layer(self):
        """Index of the conv under test."""
        return 2 if self.has_1x1 else 1

    @property
    def stored_layer(self):
        """Index of the layer that holds the conv's stored output (the shortcut when one is fused into its epilogue)."""
        return self.conv_layer + (1 if self.shortcut else 0)

    def cfg(self):
        assert not self.shortcut or (self.cin == self.cout and self.stride == 1)
        L = _net(self.H, self.W)
        L += _conv(self.stem, 3, 1)
        if self.has_1x1:
            L += _conv(self.cin, 1, 1)
        L += _conv(self.cout, self.k, self.stride, act=self.act)
        if self.shortcut:
            L += _shortcut(-2)
        L += _conv(3 * (5 + CLASSES), 1, 1, bn=False, act="linear") + _yolo((0, 1, 2), _ANCHORS_V3, 9, CLASSES)
        return "\n".join(L) + "\n"


def _p(name, shape, B, note, **kw):
    return Probe(name, *shape, B, note=note, **kw)


PROBES = [
    _p("w94_c32", (5, 94, 32, 64, 3, 1), 3, "W = BAND_MAX_W, one K chunk; 470 pixels per frame: a frame boundary in every M tile, 2 rows in the last 128-row tile"),
    _p("w94_one_row", (1, 94, 32, 64, 3, 1), 5, "one-row images: every tap row above and below is padding"),
    _p("w94_c96", (5, 94, 96, 128, 3, 1), 3, "three K chunks (odd), two N tiles"),
    _p("w33_c96", (7, 33, 96, 64, 3, 1), 3, "three K chunks (odd), one N tile"),
    _p("w33_c96_shortcut", (7, 33, 96, 96, 3, 1), 3, "three K chunks (odd) with the fused shortcut, Cout 96: no multiple of 64", shortcut=True),
    _p("hw400_c512", (20, 20, 512, 64, 3, 1), 1, "H W = 400: the two-K-group band tiles"),
    _p("hw420_c512", (21, 20, 512, 64, 3, 1), 1, "H W = 420: the one-group band tiles"),
    _p("w95_c32", (5, 95, 32, 64, 3, 1), 3, "lower end of the wide bandd tile; patch tiles, weights resident"),
    _p("w160_c32", (3, 160, 32, 128, 3, 1), 2, "upper end of the wide bandd tile; patch tiles"),
    _p("w161_c32", (4, 161, 32, 64, 3, 1), 2, "one past the wide bandd tile: patch tiles only"),
    _p("slab_c64", (9, 21, 64, 32, 1, 1), 3, "1x1 slab tiles, one 64-channel slab, Cout below the tile width; 567 pixels "
       "(fuse_pointwise off: the 32 -> 64 conv before it would host a 64 -> 32 1x1 in its epilogue and the launch under test would not run)",
       options=(("fuse_pointwise", 0),)),
    _p("slab_c192", (9, 21, 192, 96, 1, 1), 3, "1x1 slab tiles, three slabs, Cout no multiple of the tile width"),
    _p("pw_c96", (9, 21, 96, 32, 1, 1), 3, "a 1x1 layer the slab family must refuse (Cin % 64 != 0): generic / ring"),
    _p("s2_c64", (10, 22, 64, 96, 3, 2), 3, "stride 2 onto a 5x11 map: generic / ring"),
    _p("w33_c96_silu", (7, 33, 96, 64, 3, 1), 3, "SiLU in the LDS-transposed epilogue", act="silu"),
    _p("w33_c96_linear", (7, 33, 96, 64, 3, 1), 3, "linear activation", act="linear"),
    _p("narrow_c16", (9, 21, 16, 32, 3, 1), 3, "Cin = 16 from a 16-filter stem", options=(("narrow_cin", 1),)),
    _p("ks_pw_c256", (9, 21, 256, 96, 1, 1), 3, "K-sliced 1x1: 8 chunks in slices of 2", options=(("k_slices_split", 1),)),
    _p("ks_c64", (9, 21, 64, 64, 3, 1), 3, "K-sliced 3x3: 18 chunks in slices of 4, the last of 2", options=(("k_slices_split", 1),)),
    _p("ks_c64_shortcut", (9, 21, 64, 64, 3, 1), 3, "K-sliced 3x3 with the fused shortcut: the shortcut operand in the reduce kernel / the last slice's epilogue",
       options=(("k_slices_split", 1),), shortcut=True),
]
BY_NAME = {p.name: p for p in PROBES}


_setups = {}


def setup(probe):
    """(oracle with the synthetic weights loaded, weight stream, frames [B,3,H,W]) of a probe: built once."""
    if probe.name not in _setups:
        import torch
        from oracle import darknet_ref as O
        from realtimeobjectdetection_amd import synth
        from rect_ref import synth_frames_rect
        ref = O.RefDarknet(probe.cfg(), probe.H, probe.W)
        wts = synth.synth_weights(ref.ir)
        ref.load_weight_stream(wts)
        _setups[probe.name] = (ref, wts, torch.from_numpy(synth_frames_rect(probe.B, probe.H, probe.W, seed=11)))
    return _setups[probe.name]


class ProbePlan:
    """A plan of one probe through the C ABI alone (no device, no weights, nothing launched), keep_all_layers like the GPU tests."""

    def __init__(self, probe, precision, max_batch=None):
        self.lib = _ffi.lib()
        self.h = C.c_void_p()
        t = probe.cfg().encode()
        _ffi.check(self.lib.rtod_plan_create_rect(t, len(t), probe.H, probe.W, max_batch or probe.B, 0, C.byref(self.h)))
        try:
            _ffi.check(self.lib.rtod_plan_set_keep_all_layers(self.h, 1))
            for name, value in probe.options:
                _ffi.check(self.lib.rtod_plan_set_option(self.h, name.encode(), value))
            _ffi.check(self.lib.rtod_plan_set_precision(self.h, precision))
            info = _ffi.PlanInfo()
            _ffi.check(self.lib.rtod_plan_get_info(self.h, C.byref(info)))
            self.n = info.n_launches
        except Exception:
            self.close()
            raise

    def close(self):
        if self.h:
            self.lib.rtod_plan_destroy(self.h)
            self.h = C.c_void_p()

    def launches(self):
        out = []
        for i in range(self.n):
            li = _ffi.LaunchInfo()
            _ffi.check(self.lib.rtod_plan_get_launch(self.h, i, C.byref(li)))
            out.append(li)
        return out


def launch_of_layer(launch_infos, layer):
    """Index of the conv launch (kind 0) of ``layer`` in a plan's launch list."""
    hits = [i for i, li in enumerate(launch_infos) if li.kind == 0 and li.layer == layer]
    assert len(hits) == 1, (layer, [(li.layer, li.kind) for li in launch_infos])
    # a split-f16 tile of its own: not the guest of a hosted 1x1 epilogue (reported without a variant: its launch is skipped)
    assert launch_infos[hits[0]].variant >= 100, (layer, launch_infos[hits[0]].variant)
    return hits[0]


def accepted_ids(lib, handle, n_launches, launch, batch):
    """Tile ids that rtod_plan_set_tiles accepts in entry ``launch`` of an otherwise heuristic table of ``batch``; leaves an
    all-heuristic table of that batch behind."""
    table = (C.c_int * n_launches)(*([-1] * n_launches))
    ok = []
    for v in IDS:
        table[launch] = v
        if lib.rtod_plan_set_tiles(handle, batch, table, n_launches) == 0:
            ok.append(v)
    table[launch] = -1
    _ffi.check(lib.rtod_plan_set_tiles(handle, batch, table, n_launches))
    return ok


def legal_ids(probe, precision):
    """Tile ids the conv under test may run in ``precision`` (1: f16s3, 2: f16) at the probe's batch."""
    plan = ProbePlan(probe, precision)
    try:
        return accepted_ids(plan.lib, plan.h, plan.n, launch_of_layer(plan.launches(), probe.conv_layer), probe.B)
    finally:
        plan.close()
