"""Host-side mirror of the reference's validator (``DarknetValidator``, test.py:13-313) on librtod.so.

Same attribute and method names and return conventions as the reference; the scoring itself (class / size filters, thresholded
IoU matrix, greedy matching, TP / FP / FN) runs in one kernel launch per batch (``rtod_score_detections``), at any batch size,
with no host round trip per box pair.  As committed the reference's ``compare_boxes`` raises ``TypeError`` (its two helpers are
``@staticmethod``s declared with a ``self`` parameter); what is mirrored is what those helpers compute when called directly.

* ``DarknetValidator.validate_model(model, batches, CUDA=True, img_scores=False)``   test.py:244-280
* ``DarknetValidator.validate_json(pred_dict, targets_by_name, img_scores=True)``    test.py:282-313
* ``DarknetValidator.sweep(model, batches, nms_thresholds=None, confidences=None)``  the ROC loop, test.py:330-355, one forward per batch
* ``CocoTargets(annotations_json, img_dir, resolution)``                             target geometry of src/dataset.py:227-312

Scoring needs CUDA (ROCm) tensors; there is no CPU fallback.
"""
import ctypes as C
import json
import os

import torch

from . import _ffi
from .util import _need_cuda, prep_frames, write_results_async


def score_limits():
    """``(max kept predictions, max kept targets)`` per image of rtod_score_detections."""
    p, t = C.c_int(), C.c_int()
    _ffi.check(_ffi.lib().rtod_score_detections_limits(C.byref(p), C.byref(t)))
    return p.value, t.value


def _class_mask(permitted_classes, num_classes):
    words = (C.c_uint32 * ((int(num_classes) + 31) // 32))()
    for c in permitted_classes:
        c = int(c)
        if 0 <= c < int(num_classes):
            words[c >> 5] |= 1 << (c & 31)
    return words


def _score_workspace(dev, batch, cap, max_targets):
    return _ffi.workspace("rtod_score_detections", dev, batch, cap, max_targets)


def score_detections_async(rows, counts, targets, num_class, permitted_classes=(0,), min_box_size=24, iou_threshold=0.5,
                           totals=None, status=None, corners=False):
    """Enqueue rtod_score_detections for one batch; nothing synchronises.  ``rows`` / ``counts``: the device tensors of
    ``write_results_async``; ``targets``: one ``[T_i, 5+num_class]`` tensor (or None / empty) per image.  ``totals`` (int32 [4],
    accumulated) and ``status`` (int32 [1], OR-ed) are caller-owned device tensors or None.
    Returns ``(scores int32 [B,4] = people_num, tp, fp, fn;  match int32 [cap];  match_iou float32 [cap];  status)``."""
    _need_cuda(rows, "score_detections")
    if not isinstance(counts, torch.Tensor) or not counts.is_cuda or counts.dtype != torch.int32:
        raise RuntimeError("score_detections: counts must be the CUDA (ROCm) int32 tensor of write_results_async; this build has no CPU path")
    dev = rows.device
    B = len(targets)
    if rows.dim() != 2 or rows.size(1) != 8 or not rows.is_contiguous() or counts.numel() < 2 + B:
        raise ValueError("score_detections: expected rows [cap,8] and counts [>= 2 + %d]" % B)
    cap = rows.size(0)
    attrs = 5 + int(num_class)
    offs, parts = [0], []
    for t in targets:
        t = None if t is None or isinstance(t, int) else torch.as_tensor(t, dtype=torch.float32)
        if t is not None and t.numel():
            parts.append(t.reshape(-1, attrs))
        offs.append(offs[-1] + (parts[-1].size(0) if t is not None and t.numel() else 0))
    if parts and all(p.is_cuda for p in parts):
        tgt = torch.cat(parts).contiguous()
    elif parts:
        tgt = torch.cat([p.cpu() for p in parts]).contiguous().pin_memory().to(dev, non_blocking=True)
    else:
        tgt = torch.zeros((1, attrs), dtype=torch.float32, device=dev)
    toff = torch.tensor(offs, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
    max_tgt = score_limits()[1]
    ws, nbytes = _score_workspace(dev, B, cap, max_tgt)
    scores = torch.empty((B, 4), dtype=torch.int32, device=dev)
    match = torch.empty((cap,), dtype=torch.int32, device=dev)
    miou = torch.empty((cap,), dtype=torch.float32, device=dev)
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    _ffi.enqueue("rtod_score_detections", dev, rows, counts, cap, B, tgt, toff, int(num_class), _class_mask(permitted_classes, num_class),
                 float(min_box_size), float(iou_threshold), max_tgt, 1 if corners else 0, scores, totals, match, miou, status, ws, nbytes)
    return scores, match, miou, status


class CocoTargets:
    """COCO ground truth with the reference's target geometry (``COCO`` of src/dataset.py:179-338), host only (PIL and json).

    Iterating yields ``(names, frames uint8 [B,H,W,3] RGB, targets)``: consecutive images of one size share a batch of up to
    ``batch_size``; ``targets[i]`` is a float32 ``[T_i, 85]`` tensor of centre-form rows ``(cx, cy, w, h, 1, one-hot class)`` in
    network-input pixels — ``coco2yolo`` labels, ratio and pad of ``configure_padding``, rows of ``fetch_bounding_boxes`` — or an
    empty ``[0, 85]`` tensor.  The frames go through ``prep_frames(mode="RGB")`` in ``DarknetValidator.validate_model``."""

    deleted_cls = [12, 26, 29, 30, 45, 66, 68, 69, 71, 83, 91]

    def __init__(self, annotations_json, img_dir, resolution=416, batch_size=8, non_crowd=True):
        self.resolution = resolution
        self.img_dir = img_dir if img_dir.endswith("/") else img_dir + "/"
        self.batch_size = int(batch_size)
        with open(annotations_json) as f:
            ann = json.load(f)
        ids = [a["image_id"] for a in ann["annotations"] if not (non_crowd and a["iscrowd"])]
        self.img_ids = list(set(ids))                                   # the reference's order (src/dataset.py:223)
        self.img_annotations = ann["annotations"]
        self.images = {i["id"]: i for i in ann["images"]}

    def __len__(self):
        return len(self.img_ids)

    def coco2yolo(self, category_id):
        ex = 0
        for d in self.deleted_cls:
            if category_id < d:
                return category_id - ex
            ex += 1
        return category_id - ex

    def configure_padding(self, size):
        w, h = size
        max_im_size = max(w, h)
        ratio = float(self.resolution / max_im_size)
        return [int((max_im_size - w) * ratio / 2), int((max_im_size - h) * ratio / 2)], ratio

    def fetch_bounding_boxes(self, id_, pad, ratio):
        rows = []
        for annot in self.img_annotations:
            if annot["image_id"] == id_:
                cls_encoding = [1.0] + [0] * 80
                cls_encoding[self.coco2yolo(annot["category_id"])] = 1.0
                box = torch.FloatTensor(list(annot["bbox"][:5]) + cls_encoding)
                box[:4] *= ratio
                box[0] += box[2] / 2 + pad[0]
                box[1] += box[3] / 2 + pad[1]
                rows.append(box)
        return torch.stack(rows, dim=0) if rows else torch.zeros((0, 85), dtype=torch.float32)

    def _open(self, id_):
        from PIL import Image
        return Image.open(self.img_dir + self.images[id_]["file_name"])

    def targets(self, index):
        """``(file name, targets)`` of image ``index`` without decoding its pixels (the reference's only_ground_truth mode)."""
        id_ = self.img_ids[index]
        with self._open(id_) as im:
            pad, ratio = self.configure_padding(im.size)
        return self.images[id_]["file_name"], self.fetch_bounding_boxes(id_, pad, ratio)

    def targets_by_name(self):
        return dict(self.targets(i) for i in range(len(self)))

    def __iter__(self):
        import numpy as np
        names, frames, targets = [], [], []
        for id_ in self.img_ids:
            with self._open(id_) as im:
                pad, ratio = self.configure_padding(im.size)
                frame = torch.from_numpy(np.asarray(im.convert("RGB"), dtype=np.uint8).copy())
            if frames and (frame.shape != frames[0].shape or len(frames) == self.batch_size):
                yield names, torch.stack(frames), targets
                names, frames, targets = [], [], []
            names.append(self.images[id_]["file_name"])
            frames.append(frame)
            targets.append(self.fetch_bounding_boxes(id_, pad, ratio))
        if frames:
            yield names, torch.stack(frames), targets


class DarknetValidator:
    """Darknet YOLO network validator (reference: test.py:13-313).

    Attributes (the reference's): confidence, nms_thresh, validation_thresh, resolution, num_classes, image_scores,
    total_scores; after a run precision, recall, f_score (float32 tensors; 0 / 0 gives nan, as there).  New:
    ``permitted_classes`` and ``min_box_size``, the literals the reference hard-codes in validate_model (``[0]``, 24)."""

    def __init__(self, annotation_dir=None, img_dir=None, confidence=0.6, num_classes=80, nms_thresh=0.5,
                 validation_thresh=0.5, resolution=416, permitted_classes=(0,), min_box_size=24):
        assert isinstance(resolution, int) and resolution % 32 == 0
        assert confidence <= 1 and confidence >= 0
        assert nms_thresh <= 1 and nms_thresh >= 0
        self.confidence = confidence
        self.nms_thresh = nms_thresh
        self.validation_thresh = validation_thresh
        self.resolution = resolution
        self.num_classes = int(num_classes)
        self.permitted_classes = tuple(int(c) for c in permitted_classes)
        self.min_box_size = min_box_size
        self.dataset = None
        self.data_num = 0
        if annotation_dir is not None:
            self.set_dataloader(annotation_dir, img_dir)
        self.image_scores = {}
        self.total_scores = {"people_num": 0, "tp": 0, "fn": 0, "fp": 0}

    def set_dataloader(self, annotation_dir, img_dir):
        assert isinstance(annotation_dir, str)
        assert isinstance(img_dir, str)
        self.dataset = CocoTargets(annotation_dir, img_dir, self.resolution)
        self.data_num = len(self.dataset)
        self.dataloader = self.dataset

    # ------------------------------------------------------------------ the reference's per-image methods
    def target_filter(self, target, permitted_classes, min_box_size=0):
        """Targets wider and higher than ``min_box_size`` whose class is permitted, as corner boxes (xywh2xyxy), or ``None``."""
        if target is None or len(target) == 0:
            return None
        t = torch.as_tensor(target)
        cls = torch.argmax(t[:, 5:], dim=1)
        ok = torch.zeros_like(cls, dtype=torch.bool)
        for c in permitted_classes:
            ok |= cls == int(c)
        keep = (t[:, 2] > min_box_size) & (t[:, 3] > min_box_size) & ok
        if not bool(keep.any()):
            return None
        k = t[keep]
        out = k.clone()
        out[:, 0] = k[:, 0] - k[:, 2] / 2
        out[:, 1] = k[:, 1] - k[:, 3] / 2
        out[:, 2] = k[:, 0] + k[:, 2] / 2
        out[:, 3] = k[:, 1] + k[:, 3] / 2
        return out

    def pred_filter(self, pred, permitted_classes):
        """Detection rows whose class (last column) is permitted, or the int ``0``."""
        if type(pred) == int:
            return 0
        ok = torch.zeros(pred.size(0), dtype=torch.bool, device=pred.device)
        for c in permitted_classes:
            ok |= pred[:, -1] == c
        return pred[ok] if bool(ok.any()) else 0

    def compare_boxes(self, pred, target, threshold: float):
        """True positives of one image: ``pred`` detection rows ``[P, >=5]`` (box in columns 1-4), ``target`` corner boxes
        ``[T, >=4]`` (the output of target_filter), matched greedily at IoU > ``threshold`` by the kernel.  One host sync."""
        _need_cuda(pred, "compare_boxes")
        _need_cuda(target, "compare_boxes")
        P, T = pred.size(0), target.size(0)
        max_p, max_t = score_limits()
        if P > max_p or T > max_t:
            raise ValueError("compare_boxes: %d predictions / %d targets exceed the kernel's limits (%d / %d)" % (P, T, max_p, max_t))
        rows = torch.zeros((max(P, 1), 8), dtype=torch.float32, device=pred.device)
        rows[:P, 1:5] = pred[:, 1:5]
        tg = torch.zeros((T, 6), dtype=torch.float32, device=pred.device)
        tg[:, :4] = target[:, :4]
        tg[:, 4:] = 1.0
        counts = torch.tensor([P, P, P, 0], dtype=torch.int32).to(pred.device)
        scores, _, _, status = score_detections_async(rows, counts, [tg], 1, (0,), float("-inf"), threshold, corners=True)
        host = torch.cat([scores.reshape(-1), status]).cpu()
        if int(host[4]) != 0:
            raise RuntimeError("compare_boxes: rtod_score_detections status %d" % int(host[4]))
        return int(host[1])

    def save_img_scores_(self, img_name, people_num, tp, fp, fn):
        self.image_scores[img_name] = {"people_num": people_num, "tp": tp, "fp": fp, "fn": fn}

    def save_total_scores_(self, people_num, tp, fp, fn):
        self.total_scores["people_num"] += people_num
        self.total_scores["tp"] += tp
        self.total_scores["fp"] += fp
        self.total_scores["fn"] += fn

    def get_img_scores(self, img_name, pred, target, img_scores=False):
        """Scores of one image from FILTERED predictions (tensor or ``0``) and targets (corner boxes or ``None``)."""
        true_positive = false_positive = people_num = 0
        if type(pred) == int and target is None:
            return
        elif type(pred) == int:
            people_num = target.size(0)
        elif target is None:
            false_positive = pred.size(0)
        else:
            people_num = target.size(0)
            true_positive = self.compare_boxes(pred, target, self.validation_thresh)
            false_positive = pred.size(0) - true_positive
        false_negative = people_num - true_positive
        if img_scores:
            self.save_img_scores_(img_name, people_num, true_positive, false_positive, false_negative)
        self.save_total_scores_(people_num, true_positive, false_positive, false_negative)

    def save_scores(self, img_score_dir=None, total_score_dir=None):
        if img_score_dir is not None:
            json.dump(self.image_scores, open(img_score_dir, "w"))
        if total_score_dir is not None:
            json.dump(self.total_scores, open(total_score_dir, "w"))

    # ------------------------------------------------------------------ batched scoring
    def score_batch(self, rows, counts, targets, totals=None, status=None):
        """Score one batch on the device: ``rows`` / ``counts`` from ``write_results_async``, ``targets`` a list of per-image
        ``[T_i, 5+C]`` tensors.  Returns ``(scores int32 [B,4] = people_num, tp, fp, fn, match int32 [cap])`` as device tensors
        without synchronising; ``match[r]``: -2 filtered out, -1 false positive, else the index of the matched target."""
        scores, match, _, _ = score_detections_async(rows, counts, targets, self.num_classes, self.permitted_classes, self.min_box_size,
                                                     self.validation_thresh, totals=totals, status=status)
        return scores, match

    def _network_input(self, model, samples):
        x = torch.as_tensor(samples)
        if x.dtype == torch.uint8:                                       # [B,H,W,3] RGB frames: letterboxed on the device
            h = int(model.net_info["height"])
            w = int(model.input_width) if getattr(model, "input_width", None) is not None else h
            return prep_frames(x, (w, h), mode="RGB")
        return x.cuda() if not x.is_cuda else x

    def _finish(self):
        tp = torch.tensor(self.total_scores["tp"]).float()
        fp = torch.tensor(self.total_scores["fp"]).float()
        fn = torch.tensor(self.total_scores["fn"]).float()
        self.precision = (tp / (tp + fp)).clone()
        self.recall = (tp / (tp + fn)).clone()
        self.f_score = (2 / ((1 / self.recall) + (1 / self.precision))).clone()

    def _run(self, model, batches, settings, img_scores, trainer=None):
        """Shared body of validate_model and sweep: per batch ONE forward, then per (confidence, nms) setting write_results +
        scoring with that setting's device totals.  Host synchronisations: one at the end (img_scores: one per batch).
        ``trainer`` (validate_model(loss=True)): the forward runs under ``train_mode()``, the loss of the batch is added to a
        device sum, and ``finish_decode`` turns the tensor into the eval decode before write_results."""
        from .darknet import take_pending_overflow, raise_overflow
        S = len(settings)
        totals = status_log = None
        loss_sum, n_batches = None, 0
        pending, guard = [], None                                        # pending: (samples, targets, status tensor [S]) per batch

        def enqueue(x, targets, conf, nms, tot, st, cap=None):
            rows, counts = write_results_async(x, self.num_classes, conf, nms, cap=cap)
            return self.score_batch(rows, counts, targets, totals=tot, status=st)

        def settle(entries):
            """After a synchronisation: statuses of these batches; a batch that overflowed write_results' default capacity
            (status 1, nothing added to the totals) is redone at full capacity."""
            nonlocal guard
            host = torch.stack([e[2] for e in entries]).cpu() if entries else torch.zeros((0, S), dtype=torch.int32)
            if guard is not None and int(guard[1].reshape(-1)[0].item()) != 0:
                raise_overflow(guard[0])
            redo = []
            for e, st in zip(entries, host.tolist()):
                for s, v in enumerate(st):
                    if v & 2:
                        raise RuntimeError("validate: an image has more kept predictions / targets than rtod_score_detections matches %r" % (score_limits(),))
                    if v & 1:
                        redo.append((e, s))
            out = {}
            for e, s in redo:
                with torch.no_grad():
                    pred = model(self._network_input(model, e[0]))
                take_pending_overflow(pred)
                st = torch.zeros(1, dtype=torch.int32, device=pred.device)
                sc, _ = enqueue(pred, e[1], settings[s][0], settings[s][1], totals[s], st, cap=pred.size(0) * pred.size(1))
                if int(st.item()) != 0:
                    raise RuntimeError("validate: rtod_score_detections status %d at full capacity" % int(st.item()))
                out[(id(e), s)] = sc
            return out

        for names, samples, targets in batches:
            with torch.no_grad():
                if trainer is None:
                    pred = model(self._network_input(model, samples))
                else:
                    with model.train_mode():
                        pred = model(self._network_input(model, samples))
                    comp = trainer.loss_from_boxes(pred, targets)[1]
                    loss_sum = comp.clone() if loss_sum is None else loss_sum.add_(comp)
                    n_batches += 1
                    model.finish_decode(pred)
            m, flag = take_pending_overflow(pred)                        # split-f16 range guard, read at the synchronisation below
            if m is not None:
                guard = (m, flag)
            if totals is None:
                totals = torch.zeros((S, 4), dtype=torch.int32, device=pred.device)
            st = torch.zeros(S, dtype=torch.int32, device=pred.device)
            entry = (samples, targets, st)
            scores = None
            for s, (conf, nms) in enumerate(settings):
                scores, _ = enqueue(pred, targets, conf, nms, totals[s], st[s:s + 1])
            if img_scores:                                               # one synchronisation per batch (S == 1)
                host = scores.cpu()
                redone = settle([entry])
                if redone:
                    host = redone[(id(entry), 0)].cpu()
                for name, row in zip(names, host.tolist()):
                    self.save_img_scores_(name, *row)
            else:
                pending.append(entry)
        if totals is None:
            return [[0, 0, 0, 0] for _ in settings]
        torch.cuda.current_stream(totals.device).synchronize()           # THE host synchronisation of a run
        settle(pending)
        if trainer is not None:
            self.loss_components = (loss_sum / n_batches).cpu()
            self.loss = float(self.loss_components[0])
            self.loss_status = int(trainer.status.item())
        return totals.cpu().tolist()

    def validate_model(self, model, batches=None, CUDA=True, img_scores=False, loss=False):
        """Validate a detector against ground truth (reference: test.py:244-280).  ``batches``: any iterable of
        ``(names, samples, targets)`` at any batch size — ``samples`` float32 ``[B,3,H,W]`` network inputs or uint8 ``[B,H,W,3]``
        RGB frames, ``targets`` one ``[T_i, 5+C]`` centre-form tensor per image; default: the ``CocoTargets`` of the constructor.
        Per batch: forward, ``write_results_async``, ``score_batch``; the totals accumulate on the device and are read in ONE
        host synchronisation at the end of the run (``img_scores``: one per batch, to fill ``image_scores``).  At that point the
        split-f16 range flag is honoured like ``write_results`` honours it, and a batch whose detections exceeded
        ``write_results_async``'s default capacity is redone at full capacity (its ``samples`` are kept until then).
        The frames of a batch are independent only with ``model.eval()``: in training mode BatchNorm runs on the statistics of
        the batch (as in the reference, which never calls ``.eval()`` and therefore validates at batch 1).
        ``loss=True`` also evaluates the reference's training loss (train.DarknetTrainer.loss_from_boxes) of every batch against
        its targets, still with ONE forward per batch: it runs under ``train_mode()``, the loss is added to a sum on the device,
        ``Darknet.finish_decode`` turns the tensor into the eval decode in place (bit-identical to an eval forward), and
        write_results and the scoring go on as before.  After the run ``loss`` is the mean loss per batch (a float, like the
        reference's ``history['train_loss']``), ``loss_components`` the float64 [6] means (total, xy, wh, obj, noobj, cls) and
        ``loss_status`` the trainer's status word (bit 0: a box lay outside a grid and was skipped).  ``loss=False`` launches
        nothing new."""
        if not CUDA:
            raise RuntimeError("DarknetValidator.validate_model: this build has no CPU path (CUDA=False)")
        if batches is None:
            batches = self.dataset
        trainer = None
        if loss:
            from .train import DarknetTrainer
            trainer = DarknetTrainer(model, num_classes=self.num_classes)
            trainer.min_box_size = self.min_box_size
            self.loss, self.loss_components, self.loss_status = float("nan"), None, 0
        people, tp, fp, fn = self._run(model, batches, [(self.confidence, self.nms_thresh)], img_scores, trainer)[0]
        self.save_total_scores_(people, tp, fp, fn)
        self._finish()
        print("\tPrecision = ", self.precision)
        print("\tRecall = ", self.recall)
        print("\tF_Score = ", self.f_score)
        if loss:
            print("\tLoss = ", self.loss)

    def validate_json(self, pred_dict, targets_by_name=None, img_scores=True, batch_size=64, device=None):
        """The same from stored detections (reference: test.py:282-313): ``pred_dict`` maps an image name to its detection rows
        ``[D, 8]`` (a dict, or the path of a JSON file), ``targets_by_name`` the name to its ``[T, 5+C]`` targets (default: the
        constructor's dataset).  One launch per ``batch_size`` images, one host synchronisation at the end."""
        if isinstance(pred_dict, str):
            pred_dict = json.load(open(pred_dict, "r"))
        if targets_by_name is None:
            targets_by_name = self.dataset.targets_by_name()
        if not torch.cuda.is_available():
            raise RuntimeError("DarknetValidator.validate_json: this build has no CPU path")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        names = list(targets_by_name)
        totals = torch.zeros(4, dtype=torch.int32, device=dev)
        done = []
        for i in range(0, len(names), batch_size):
            chunk = names[i:i + batch_size]
            rows = [torch.as_tensor(pred_dict.get(n, []), dtype=torch.float32).reshape(-1, 8) for n in chunk]
            per = [r.size(0) for r in rows]
            D = sum(per)
            allrows = torch.cat(rows + [torch.zeros((1, 8))]).pin_memory().to(dev, non_blocking=True)
            counts = torch.tensor([D, D] + per + [0, 0], dtype=torch.int32).pin_memory().to(dev, non_blocking=True)
            st = torch.zeros(1, dtype=torch.int32, device=dev)
            scores, _ = self.score_batch(allrows, counts, [targets_by_name[n] for n in chunk], totals=totals, status=st)
            done.append((chunk, scores, st))
        host_tot = totals.cpu().tolist()                                 # the host synchronisation
        for chunk, scores, st in done:
            if int(st.item()) != 0:
                raise RuntimeError("validate_json: rtod_score_detections status %d (limits %r kept predictions / targets per image)" % (int(st.item()), score_limits()))
            if img_scores:
                for n, row in zip(chunk, scores.cpu().tolist()):
                    self.save_img_scores_(n, *row)
        self.save_total_scores_(*host_tot)
        self._finish()
        print("\tPrecision = ", self.precision)
        print("\tRecall = ", self.recall)
        print("\tF_Score = ", self.f_score)

    def sweep(self, model, batches=None, nms_thresholds=None, confidences=None):
        """The threshold sweep behind the reference's ROC plot (test.py:330-355) without its 19 passes over the dataset: ONE
        forward per batch, then per setting ``write_results_async`` + scoring on the same prediction tensor, per-setting totals
        on the device, one host synchronisation at the end.  Settings: every ``nms_thresholds`` value (default: the reference's
        ``0.05 * i, i = 19 .. 1``) at ``self.confidence``, or every ``confidences`` value at ``self.nms_thresh``, or their
        product (confidence-major) when both are given.  Returns one dict per setting (confidence, nms_thresh, tp, fp, fn,
        people_num, precision, recall, f_score), equal to a fresh validator run per setting.  Leaves ``total_scores`` alone."""
        if nms_thresholds is None and confidences is None:
            nms_thresholds = [0.05 * i for i in range(19, 0, -1)]
        confs = [self.confidence] if confidences is None else list(confidences)
        nmss = [self.nms_thresh] if nms_thresholds is None else list(nms_thresholds)
        settings = [(c, n) for c in confs for n in nmss]
        if batches is None:
            batches = self.dataset
        out = []
        for (conf, nms), (people, tp_, fp_, fn_) in zip(settings, self._run(model, batches, settings, False)):
            tp, fp, fn = torch.tensor(tp_).float(), torch.tensor(fp_).float(), torch.tensor(fn_).float()
            precision, recall = tp / (tp + fp), tp / (tp + fn)
            out.append({"confidence": conf, "nms_thresh": nms, "tp": tp_, "fp": fp_, "fn": fn_, "people_num": people,
                        "precision": precision, "recall": recall, "f_score": 2 / ((1 / recall) + (1 / precision))})
        return out
