"""What tests/test_loss_host.py and tests/test_loss_gpu.py share: the cases of tests/golden/yolo_loss.npz with their prediction
tensors regenerated from the recorded seed, and the comparison of a dense target with a case."""
import os
import zlib

import numpy as np

import loss_ref as R

F = np.float32


def make_pred(seed, B, N, attrs=85):
    """The generator's prediction tensor (tests/golden/make_golden_loss.py): RandomState's frozen stream, columns 2-3 in [-2, 2)."""
    p = np.random.RandomState(seed).random_sample((B, N, attrs)).astype(F)
    p[..., 2:4] = p[..., 2:4] * F(4) - F(2)
    return p


def load_cases(golden_dir):
    g = np.load(os.path.join(golden_dir, "yolo_loss.npz"))
    out = []
    for idx, name in enumerate(g["case_names"].tolist()):
        k = "c%d_" % idx
        c = {f: g[k + f] for f in ("heads", "anchors", "boxes", "box_offsets", "rows", "target_rows", "loss32", "loss64", "comp32", "comp64", "log_ulps", "seed", "pred_sum", "pred_crc")}
        an, heads = c["anchors"].tolist(), []
        for gh, gw, s, a in c["heads"].tolist():
            heads.append((gh, gw, s, [tuple(v) for v in an[:a]]))
            an = an[a:]
        off = c["box_offsets"].tolist()
        c.update(name=name, heads=heads, images=[c["boxes"][off[i]:off[i + 1]] for i in range(len(off) - 1)], N=sum(R.head_rows(heads)))
        c["B"] = len(c["images"])
        c["pred"] = make_pred(int(c["seed"]), c["B"], c["N"])
        assert zlib.crc32(c["pred"].tobytes()) == int(c["pred_crc"]) and c["pred"].astype(np.float64).sum() == float(c["pred_sum"]), name
        out.append(c)
    return g, out


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def check_targets(c, target, mask, tag):
    """A dense target / mask against a fixture case: rows integer-exact, columns 0, 1, 4.. bit-exact, tw / th within the recorded
    distance of the reference's values."""
    flat = np.flatnonzero(np.asarray(mask).reshape(-1))
    assert np.array_equal(flat, c["rows"]), tag
    got = np.asarray(target, F).reshape(-1, target.shape[-1])
    want = c["target_rows"]
    keep = [0, 1] + list(range(4, want.shape[1]))
    assert np.array_equal(bits(got[flat][:, keep]), bits(want[:, keep])), tag
    if len(flat):
        assert int(R.ulp_distance(got[flat][:, 2:4], want[:, 2:4]).max()) <= int(c["log_ulps"]), tag
    rest = np.ones(len(got), bool)
    rest[flat] = False
    assert not got[rest].any(), tag                                   # every other row is all zero
