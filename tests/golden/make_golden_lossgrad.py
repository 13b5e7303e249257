#!/usr/bin/env python
"""Fixture that pins the gradient of the training loss to the reference's own autograd (same harness as make_golden_loss.py):

    python tests/golden/make_golden_lossgrad.py <reference checkout>

writes tests/golden/yolo_loss_grad.npz.  Cases: the four of yolo_loss.npz, with their boxes and heads (read from that file).  Raw
head maps are drawn from a recorded RandomState seed (``standard_normal``, NCHW, head after head from one stream) and not stored:
the tests regenerate them and check the recorded checksum.  They go through the reference's ``predict_transform(TRAIN=True)`` per
head, ``torch.cat``, its ``target_creator`` and ``darknet_loss``, then ``backward()``, once in float32 and once in float64.
Recorded sparsely per case: the gradient of the objectness channel of the raw maps for every row ([B, N], row layout), the full
85-wide gradient of every object row with respect to the raw maps (dz) and to the prediction tensor (g), all in both precisions,
the two losses, and the float32 floor: rms and max of (g32 - g64) / D over the structurally non-zero elements, D as in
tests/head_grad_ref.py (the magnitude the subtraction's operands carry).  Data only: nothing from the reference is copied."""
import importlib.util
import os
import sys
import types
import zlib

import numpy as np

sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
F = np.float32
C = 80
RES = 416
SEED0 = 977


def make_raws(seed, B, heads, attrs=5 + C):
    """The frozen stream of numpy.random.RandomState: one standard-normal [B, A*attrs, GH, GW] float32 map per head, in head order."""
    rng = np.random.RandomState(seed)
    return [rng.standard_normal((B, len(an) * attrs, gh, gw)).astype(F) for gh, gw, _, an in heads]


def main(ref):
    import torch
    import torch.nn as nn
    import head_grad_ref as G
    from loss_cases import load_cases
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    sys.path.insert(0, ref)

    def load(name, fname):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ref, fname))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod

    load("test", "test.py")
    ref_train = load("ref_train", "train.py")
    from src.util import predict_transform

    def trainer(heads):
        t = ref_train.DarknetTrainer.__new__(ref_train.DarknetTrainer)
        t.num_classes, t.resolution, t.TINY = C, RES, len(heads) == 2
        t.darknet = types.SimpleNamespace(anchors=[a for _, _, _, an in heads for a in an])
        t.MSELoss = nn.MSELoss(reduction="sum")
        return t

    _, cases = load_cases(HERE)
    out = {"case_names": np.asarray([c["name"] for c in cases])}
    for idx, c in enumerate(cases):
        k = "c%d_" % idx
        heads, B, N = c["heads"], c["B"], c["N"]
        t = trainer(heads)
        bnd = [torch.from_numpy(im) if len(im) else [] for im in c["images"]]
        target, mask = t.target_creator(bnd)
        flat = np.flatnonzero(mask.numpy().reshape(-1))
        assert np.array_equal(flat, c["rows"]), c["name"]
        seed = SEED0 + idx
        raws = make_raws(seed, B, heads)
        res = {}
        for tag, dt in (("32", torch.float32), ("64", torch.float64)):
            leaves = [torch.from_numpy(r).to(dt).requires_grad_(True) for r in raws]
            pred = torch.cat([predict_transform(z, RES, an, C, False, TRAIN=True) for z, (_, _, _, an) in zip(leaves, heads)], 1)
            pred.retain_grad()
            loss = t.darknet_loss(pred, target.to(dt), mask)
            loss.backward()
            assert loss.dtype == dt and tuple(pred.shape) == (B, N, 5 + C)
            dz = np.concatenate([G.rows_from_raw(z.grad.numpy(), len(an), 5 + C) for z, (_, _, _, an) in zip(leaves, heads)], axis=1)
            res[tag] = {"loss": loss.item(), "g": pred.grad.numpy(), "dz": dz, "pred": pred.detach().numpy()}
        m = mask.numpy()
        p64, t64 = res["64"]["pred"], target.numpy().astype(np.float64)
        for tag in ("32", "64"):                                     # the zero pattern of the closed form is autograd's own
            for name in ("g", "dz"):
                v = res[tag][name].copy()
                v[m] = 0
                v[..., 4] = 0
                assert not v.any(), (c["name"], tag, name)
        # the closed form of tests/head_grad_ref.py is what float64 autograd gives
        ref64 = G.grad_pred(p64, t64, m)
        assert np.abs(ref64 - res["64"]["g"]).max() <= 1e-12 and np.abs(ref64 * G.sig_factor(p64) - res["64"]["dz"]).max() <= 1e-12
        floors = {}
        for name, raw in (("g", False), ("dz", True)):
            floors[name] = G.relative_error(res["32"][name], res["64"][name], G.scale(p64, t64, m, raw))
        sel = m.reshape(-1)
        for tag, dt in (("32", F), ("64", np.float64)):
            out[k + "dz_obj" + tag] = res[tag]["dz"][..., 4].astype(dt)
            out[k + "dz_rows" + tag] = res[tag]["dz"].reshape(-1, 5 + C)[sel].astype(dt)
            out[k + "g_rows" + tag] = res[tag]["g"].reshape(-1, 5 + C)[sel].astype(dt)
        out[k + "loss32"] = np.float32(res["32"]["loss"])
        out[k + "loss64"] = np.float64(res["64"]["loss"])
        out[k + "floor_g"] = np.asarray(floors["g"], np.float64)
        out[k + "floor_dz"] = np.asarray(floors["dz"], np.float64)
        out[k + "seed"] = np.int64(seed)
        out[k + "raw_crc"] = np.int64(zlib.crc32(b"".join(r.tobytes() for r in raws)))
        print(c["name"], "B", B, "N", N, "masked", len(flat), "non-zero", int((res["64"]["dz"] != 0).sum()), "of", res["64"]["dz"].size,
              "loss32", res["32"]["loss"], "loss64", res["64"]["loss"], "floor g rms %.3g max %.3g" % floors["g"], "floor dz rms %.3g max %.3g" % floors["dz"])
    path = os.path.join(HERE, "yolo_loss_grad.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
