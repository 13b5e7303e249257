"""GPU test that pins the bits of the LDS-staged split-f16 convs (conv_f16s3_staged.h: generic, 16-channel and K-sliced
families).  Run on an MI355X with ``pytest -m gpu``.

The generic tiles are held bit for bit to the ring, slab and patch tiles by tests/test_f16s3_local_gpu.py; a 16-channel or a
K-sliced layer runs on no other family, so their bits are compared with a record instead: tests/golden/staged_conv_bits.json,
written once by tools/dump_staged_bits.py from the library as it stood BEFORE the three kernels were moved onto the shared main
loop (its "recorded_from" names the commit).  It is not regenerated: a change of these bits is a change of the arithmetic or of
its summation order and has to be argued as such.

Per probe and precision the record holds the SHA-256 of the float32 bytes of read_layer(stored_layer) of the conv under test on
the heuristic tile (autotune off), and the tile id that ran.  The decoded output is not hashed: its hardware exp is not what is
pinned here.
"""
import hashlib
import json
import os

import pytest
import torch

from realtimeobjectdetection_amd import cfgs
from conv_probes import BY_NAME, launch_of_layer, setup

pytestmark = pytest.mark.gpu

PROBES = ["narrow_c16", "ks_pw_c256", "ks_c64", "s2_c64", "pw_c96"]
PRECISIONS = ["f16s3", "f16"]
RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "staged_conv_bits.json")


def digest(name, precision, d):
    """{"tile": id that ran, "sha256": of the stored layer's float32 bytes} of one probe on its heuristic tile."""
    from realtimeobjectdetection_amd.darknet import Darknet
    p = BY_NAME[name]
    _, wts, x = setup(p)
    m = Darknet(cfgs.write_cfg(os.path.join(str(d), "net.cfg"), p.cfg()), True).eval()
    m.net_info["height"] = p.H
    m.input_width = p.W
    m.precision = precision
    m.options = dict(p.options)
    m.keep_all_layers = True
    m.autotune = False
    m.load_weight_stream(wts)
    with torch.no_grad():
        m(x.cuda())
    torch.cuda.synchronize()
    assert m.active_precision == precision and not m.overflowed(), (name, precision)
    li = m.launch_infos()
    t = m.read_layer(p.stored_layer, p.B).cpu().float().contiguous()
    return {"tile": li[launch_of_layer(li, p.conv_layer)].variant - 100, "sha256": hashlib.sha256(t.numpy().tobytes()).hexdigest()}


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", PROBES)
def test_staged_conv_has_the_recorded_bits(tmp_path, name, precision):
    want = json.load(open(RECORD))["digests"]["%s/%s" % (name, precision)]
    got = digest(name, precision, tmp_path)
    print("STAGED %s %s: tile %d sha256 %s" % (name, precision, got["tile"], got["sha256"]))
    assert got == want
