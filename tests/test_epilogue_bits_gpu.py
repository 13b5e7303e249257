"""GPU test that pins the bits of every split-f16 conv epilogue.  Run on an MI355X with ``pytest -m gpu``.

The epilogues share their scale / bias / activation / shortcut / split / store arithmetic (the epi_* pieces of
csrc/conv_f16s3_common.h and conv_f16s3_epi_transpose.inc); this module shows that they still give the bits of the library as it
stood BEFORE those were shared: tests/golden/epilogue_bits.json,
written once by tools/dump_epilogue_bits.py (its "recorded_from" names the commit).  It is not regenerated: a change of these
bits is a change of the arithmetic and has to be argued as such.

Per probe (tests/conv_probes.py) and precision, EVERY tile id ``legal_ids`` returns for the conv under test is forced through a
tile table (autotune off); the record holds, per id, the SHA-256 of the float32 bytes of read_layer(stored_layer).  A pair whose
legal set is empty is absent from the record by construction.  Three more groups, f16s3 only:

* "raw/...": the raw-sum instances (option bn_batch_split, module in training mode), every legal id.  The mode is square-only
  (Darknet.prepare refuses a rectangular input in training mode), so these are the square probes of tests/bn_split_model.py that
  have the shapes of w33_c96 and slab_c192 (a_band96: 96 channels, three K chunks, band tiles; e_slab192: 192 -> 96 1x1, slab and
  generic tiles), and with them the two-K-group band tiles (b_band_k2) and the generic tiles on a 3x3 conv (d_wide);
* "hosted/slab_c64": slab_c64 WITH the hosted pointwise conv: the 64 -> 32 guest layer's stored output, every legal id of the host's launch;
* "stem2/...": the fused stem + layer 1 (+ hosted layer 2) kernel on YOLOv3 at 96x96, batch 3 (the case of
  test_gpu_parity.py::test_fused_stem_kernel_is_bit_identical): the layers of that kernel that are still in the arena after the forward.

The decoded output is not hashed: its hardware exp is not what is pinned here.
"""
import hashlib
import json
import os
import warnings

import pytest
import torch

from realtimeobjectdetection_amd import _ffi, cfgs, synth
from bn_split_model import BY_NAME as SQUARE_BY_NAME
from conv_probes import BY_NAME, accepted_ids, launch_of_layer, legal_ids, setup

pytestmark = pytest.mark.gpu

PROBES = ["w33_c96_shortcut", "w33_c96_silu", "w33_c96_linear", "hw400_c512", "hw420_c512", "w94_c32", "w160_c32", "slab_c192",
          "s2_c64", "pw_c96", "narrow_c16", "ks_pw_c256", "ks_c64", "ks_c64_shortcut"]
PRECISIONS = ["f16s3", "f16"]
RAW_PROBES = ["a_band96", "b_band_k2", "d_wide", "e_slab192"]
STEM2_RES, STEM2_B, STEM2_LAYERS = 96, 3, (1, 2)
RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "epilogue_bits.json")


def _sha(t):
    return hashlib.sha256(t.cpu().float().contiguous().numpy().tobytes()).hexdigest()


def _darknet(cfg_text, h, w, precision, options, d, wts, train=False):
    from realtimeobjectdetection_amd.darknet import Darknet
    m = Darknet(cfgs.write_cfg(os.path.join(str(d), "net.cfg"), cfg_text), True)
    if not train:
        m.eval()
    m.net_info["height"] = h
    if w != h:
        m.input_width = w
    m.precision = precision
    m.options = dict(options)
    m.keep_all_layers = True
    m.autotune = False
    m.update_running_stats = False
    m.load_weight_stream(wts)
    return m


def _forward(m, xg):
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                      # the training-mode warning
        m(xg)
    torch.cuda.synchronize()


def digests(name, precision, d, raw=False, hosted=False):
    """{str(tile id): sha256 of the stored layer} of one probe: every id rtod_plan_set_tiles accepts for the launch under test.
    raw: option bn_batch_split, training mode.  hosted: the probe's fuse_pointwise = 0 dropped; the launch under test is the
    host's (the 1x1 before the conv under test), the layer hashed the guest's."""
    p = (SQUARE_BY_NAME if raw else BY_NAME)[name]
    _, wts, x = setup(p)
    xg = x.cuda()
    options = dict(() if hosted else p.options)
    if raw:
        options["bn_batch_split"] = 1
    m = _darknet(p.cfg(), p.H, p.W, precision, options, d, wts, train=raw)
    m.prepare(p.B, xg.device)
    assert m.active_precision == precision, (name, precision)
    n = m._info.n_launches
    launch = launch_of_layer(m.launch_infos(), p.conv_layer - 1 if hosted else p.conv_layer)
    ids = accepted_ids(_ffi.lib(), m._plan, n, launch, p.B)
    if not raw and not hosted:
        assert ids == legal_ids(p, 1 if precision == "f16s3" else 2), (name, precision, ids)
    out = {}
    for v in ids:
        table = [-1] * n
        table[launch] = v
        m.set_tiles(p.B, table)
        _forward(m, xg)
        li = m.launch_infos()[launch]
        assert li.variant == 100 + v, (name, v, li.variant)                  # the id really ran
        if hosted:
            assert li.fused_pointwise, (name, v)
        assert not m.overflowed(), (name, v)
        out[str(v)] = _sha(m.read_layer(p.stored_layer, p.B))
    return out


def stem2_digests(d):
    """{str(layer): sha256} of the layers the fused stem kernel stores (YOLOv3 96x96, batch 3, f16s3, no keep_all_layers)."""
    from realtimeobjectdetection_amd.darknet import Darknet
    from oracle import darknet_ref as O
    text = cfgs.yolov3_cfg(STEM2_RES, STEM2_RES)
    m = Darknet(cfgs.write_cfg(os.path.join(str(d), "yolov3.cfg"), text), True).eval()
    m.net_info["height"] = STEM2_RES
    m.precision = "f16s3"
    m.load_weight_stream(synth.synth_weights(O.RefDarknet(text, STEM2_RES).ir))
    x = torch.from_numpy(synth.synth_frames(STEM2_B, STEM2_RES, seed=5)).cuda()
    _forward(m, x)
    assert len([li for li in m.launch_infos() if li.variant == 230]) == 1 and not m.overflowed()
    return {str(i): _sha(m.read_layer(i, STEM2_B)) for i in STEM2_LAYERS}


def _record():
    return json.load(open(RECORD))["digests"]


def _check(key, got):
    want = _record()[key]
    print("EPILOGUE %s: %d ids %s" % (key, len(got), sorted(got, key=int)))
    assert sorted(got, key=int) == sorted(want, key=int), (key, "ids that ran against ids recorded")
    bad = [v for v in got if got[v] != want[v]]
    assert not bad, (key, "ids whose bits differ from the record", bad)


def _pairs():
    return [(n, p) for n in PROBES for p in PRECISIONS if legal_ids(BY_NAME[n], 1 if p == "f16s3" else 2)]


def test_the_record_holds_every_probe_precision_and_id():
    rec = _record()
    for n, p in _pairs():
        assert sorted(int(v) for v in rec["%s/%s" % (n, p)]) == legal_ids(BY_NAME[n], 1 if p == "f16s3" else 2), (n, p)
    want = {"%s/%s" % np_ for np_ in _pairs()} | {"raw/%s" % n for n in RAW_PROBES} | {"hosted/slab_c64", "stem2/yolov3_96_b3"}
    assert set(rec) == want


@pytest.mark.parametrize("name,precision", _pairs())
def test_every_tile_has_the_recorded_epilogue_bits(tmp_path, name, precision):
    _check("%s/%s" % (name, precision), digests(name, precision, tmp_path))


@pytest.mark.parametrize("name", RAW_PROBES)
def test_raw_sum_instances_have_the_recorded_bits(tmp_path, name):
    _check("raw/%s" % name, digests(name, "f16s3", tmp_path, raw=True))


def test_hosted_pointwise_conv_has_the_recorded_bits(tmp_path):
    _check("hosted/slab_c64", digests("slab_c64", "f16s3", tmp_path, hosted=True))


def test_fused_stem_kernel_has_the_recorded_bits(tmp_path):
    _check("stem2/yolov3_96_b3", stem2_digests(tmp_path))
