"""AP bookkeeping (reference future_od/utils/od_map.py): the per-batch greedy TP/FP assignment runs
as one HIP kernel (fod_od_map, one wave per sample x class x IoU threshold) instead of the
reference's 50-step tensor loop; the end-of-epoch aggregation is small host math.

The same bookkeeping over the detection ROWS `predict` returns (fod_detect_od_map, one launch): prepare_od_map_detections,
DetectionEvaluator and operating_point -- what top_k, score_threshold, per_query and the duplicate suppression do to AP,
precision and recall.  Nothing of it runs unless it is called.

StreamingDetectionEvaluator keeps integer histograms over score bins instead of every batch's tensors (fod_ap_hist_accum /
fod_ap_hist_finalize): constant memory, one all_reduce between ranks, COCO's 101-point AP and a precision / recall curve."""
import numpy as np
import torch

from future_od.native import detect

SIZE_CATEGORY_DELIMITERS = [(1 / 24) * (1 / 64), (1 / 4) * (1 / 12)]   # fractions of H*W
NUM_THRESHOLDS = 10                                                   # IoU 0.50 : 0.05 : 0.95


@torch.no_grad()
def prepare_od_map_stuffs(pred_boxes, pred_class_scores, anno_boxes, anno_classes, anno_active, imsize):
    """pred_boxes (B,M,4) xyxy px, pred_class_scores (B,M,C) incl. the generic class, dense annotations
    (B,N,*) -> confs (T,C,B*K) f32, is_positive (T,C,B*K) bool, size_categories (C,4,B*K) bool,
    num_annos (C,4) i64 with K = min(50, M) (reference od_map.py:214-287)."""
    B, M, C = pred_class_scores.shape
    N = anno_classes.shape[-1]
    return detect.od_map(pred_class_scores.detach().float().contiguous(), pred_boxes.detach().float().contiguous(),
                      anno_boxes.reshape(B, N, 4).float().contiguous(), anno_classes.reshape(B, N).contiguous(),
                      anno_active.reshape(B, N).contiguous(), imsize, T=NUM_THRESHOLDS)


def _get_ap(confs, is_positive, size_categories, num_annos):
    """One IoU threshold: confs (C,P), is_positive (C,P), size_categories (C,S,P), num_annos (C,S,iters)
    -> AP (C,S) as mean precision at the true positives (reference od_map.py:290-314)."""
    C, S, P = size_categories.shape
    order = confs.argsort(dim=1, descending=True).view(C, 1, P).expand(-1, S, -1)
    tp = (is_positive.view(C, 1, P) * size_categories).gather(2, order)
    seen = size_categories.gather(2, order)
    precision = tp.cumsum(dim=2) / (seen.cumsum(dim=2) + 1e-5)
    return (precision * tp).sum(dim=2) / num_annos.sum(dim=2)


def aggregate_mean_average_precision(confs, is_positive, size_categories, num_annos, device):
    """Stacked per-iteration intermediaries -> dict of AP tables (reference od_map.py:317-364).
    Works on any device (the reference's cuda-event timing made it GPU-only)."""
    T = confs.shape[0]
    with torch.no_grad():
        ap = torch.stack([_get_ap(confs[t].to(device), is_positive[t].to(device), size_categories.to(device),
                                  num_annos.to(device)) for t in range(T)]).cpu()
    print("Number of annos for each class and size category is:")
    print(num_annos.sum(dim=2))
    return _ap_tables(ap)


def _ap_tables(ap):
    """AP (T,C,S) on the host, the generic class last -> the tables every aggregation returns."""
    per_class = ap[:, 0:-1, :].numpy()
    return {
        "all": ap[:, 0:-1, :],
        "classavg": np.nanmean(per_class, axis=1),
        "threshavg": np.nanmean(per_class, axis=0),
        "classavg threshavg": np.nanmean(per_class, axis=(0, 1)),
        "generic": ap[:, -1, :],
        "generic threshavg": np.nanmean(ap[:, -1, :].numpy(), axis=0),
    }


DETECTION_KEYS = ("scores", "labels", "boxes", "query", "count")


@torch.no_grad()
def prepare_od_map_detections(det, anno_boxes, anno_classes, anno_active, imsize, num_classes, per_class=50):
    """`prepare_od_map_stuffs` for the dict of `predict` / `GraphedPredict` (suppressed by `nms=` or not) instead of dense
    scores: the rows below `count` in their order are the ranking, class c's candidates are its first `per_class` rows,
    the generic class's are the first row of every query (detect.detect_od_map; fod_detect_od_map in include/fod_ext.h has
    the exact semantics).  -> confs (T,C,B*P) f32, is_positive (T,C,B*P) bool, size_categories (C,4,B*P) bool, num_annos
    (C,4) i64 with C = num_classes + 1 and P = min(per_class, K).  One launch, nothing read back.  With every pair
    selected (top_k = M * num_classes, threshold 0) this is `prepare_od_map_stuffs` on the same predictions, bit for bit.
    The boxes must be in the annotations' frame: a `det` that carries a `box_map` (the batch's, or the one handed to
    `predict`) holds boxes in the camera's frame and is refused."""
    if det.get("box_map") is not None:
        raise ValueError("prepare_od_map_detections: these detections went through a box_map (boxes in the camera's "
                         "frame); the annotations are in the network's input frame")
    B, N = anno_classes.shape[0], anno_classes.shape[-1]
    return detect.detect_od_map(*(det[k] for k in DETECTION_KEYS), anno_boxes.reshape(B, N, 4).float().contiguous(),
                             anno_classes.reshape(B, N).contiguous(), anno_active.reshape(B, N).contiguous(), imsize,
                             num_classes, per_class, T=NUM_THRESHOLDS)


def operating_point(confs, is_positive, size_categories, num_annos, t=0):
    """What the returned rows ARE at IoU threshold `t` (0: IoU 0.5), with no ranking involved: per class, the generic
    class last, "detections" (the filled slots: column 0 of size_categories), "true_positives", "annotations" (i64 [C])
    and "precision" = TP / detections, "recall" = TP / annotations, "f1" = 2 TP / (detections + annotations) (f64 [C],
    NaN where the denominator is 0), plus "iou".  Takes one batch's four tensors or the concatenated ones (num_annos
    (C,4) or (C,4,iterations))."""
    filled = size_categories[:, 0].bool()
    det = filled.sum(dim=1).cpu()
    tp = (is_positive[t].bool() & filled).sum(dim=1).cpu()
    anno = (num_annos[:, 0] if num_annos.dim() == 2 else num_annos[:, 0].sum(dim=1)).cpu()
    return _operating_point(det, tp, anno, t)


def _operating_point(det, tp, anno, t):
    ratio = lambda a, b: torch.where(b > 0, a.double() / b.double().clamp(min=1), torch.full_like(a, float("nan"), dtype=torch.float64))
    return {"iou": 0.5 + 0.05 * t, "detections": det, "true_positives": tp, "annotations": anno,
            "precision": ratio(tp, det), "recall": ratio(tp, anno), "f1": ratio(2 * tp, det + anno)}


class DetectionEvaluator:
    """ev = DetectionEvaluator(num_classes); for batch: ev.update(model.predict(batch, ...), batch); ev.aggregate()

    The AP of what `predict` RETURNS over a set of labelled batches: `update` makes one launch and keeps its four device
    tensors (nothing is read back), `aggregate` concatenates them as the trainer's epoch does and returns
    `aggregate_mean_average_precision`'s dict plus "operating_point"."""

    def __init__(self, num_classes, per_class=50):
        self.num_classes, self.per_class = int(num_classes), int(per_class)
        self.reset()

    def reset(self):
        self._od = [[], [], [], []]

    def __len__(self):
        return len(self._od[0])

    def update(self, det, data):
        """`det`: the dict of `predict(data, ...)`; `data`: the batch with `boxes`, `classes`, `active` and `video`."""
        if data.get("box_map") is not None and det.get("box_map") is None:
            det = dict(det, box_map=data["box_map"])       # predict applied the batch's map
        od = prepare_od_map_detections(det, data["boxes"], data["classes"], data["active"], data["video"].shape[-2:],
                                       self.num_classes, self.per_class)
        for kept, t in zip(self._od, od):
            kept.append(t)
        return od

    def tensors(self):
        """The concatenated intermediaries: confs, is_positive, size_categories (slots of all updates) and num_annos
        (C,4,updates)."""
        if not len(self):
            raise RuntimeError("DetectionEvaluator: no update yet")
        return (torch.cat(self._od[0], dim=2), torch.cat(self._od[1], dim=2), torch.cat(self._od[2], dim=2),
                torch.stack(self._od[3], dim=2))

    def aggregate(self, device=None):
        od = self.tensors()
        ap = aggregate_mean_average_precision(*od, od[0].device if device is None else device)
        ap["operating_point"] = operating_point(*od)
        return ap


class StreamingDetectionEvaluator(DetectionEvaluator):
    """ev = StreamingDetectionEvaluator(num_classes); for batch: ev.update(model.predict(batch, ...), batch); ev.aggregate()

    DetectionEvaluator in constant memory: `update` runs the bookkeeping launch into buffers it reuses and folds them into
    integer histograms over 16257 score bins (detect.ap_hist_accum: one more launch, nothing read back, nothing kept per
    batch), so a set of any size can be scored and `tensors()` has nothing to return.  `aggregate` adds the states of
    all ranks with one all_reduce(SUM) per tensor when a process group with more than one rank is initialised (exact
    integers: every rank returns the bytes one process that saw all batches returns), finalises in one launch
    (detect.ap_hist_finalize) and returns `aggregate_mean_average_precision`'s tables from the AP taken on bins, plus
    "coco" (the same tables from the 101-point interpolated AP), "pr_curve" ("precision" f64 and "score" f32
    [T,C,4,101], "recall" = i / 100) and "operating_point" with DetectionEvaluator's fields.  Where no two candidates of a
    (class, size) row share a bin the AP is the sorted one up to f64 rounding; otherwise a bin's candidates are counted
    together.  `update_od` takes the four tensors directly, e.g. `prepare_od_map_stuffs`' of the dense path.
    (A class of its own, not a keyword of DetectionEvaluator: that constructor is kept as it is.)"""

    def reset(self):
        self._updates = 0
        if getattr(self, "_state", None) is not None:
            for t in self._state:
                t.zero_()
        else:
            self._state, self._bufs = None, {}

    def __len__(self):
        return self._updates

    def update_od(self, od):
        """One batch's (confs, is_positive, size_categories, num_annos) into the state."""
        if self._state is None:
            self._state = detect.ap_hist_state(od[0].shape[0], self.num_classes + 1, od[0].device)
        detect.ap_hist_accum(od, self._state)
        self._updates += 1
        return od

    def update(self, det, data):
        if data.get("box_map") is not None or det.get("box_map") is not None:
            raise ValueError("StreamingDetectionEvaluator: these detections went through a box_map (boxes in the camera's "
                             "frame); the annotations are in the network's input frame")
        B, N = data["classes"].shape[0], data["classes"].shape[-1]
        (_, K), dev = det["scores"].shape, det["scores"].device
        C1, P = self.num_classes + 1, min(self.per_class, K)
        out = self._bufs.get((B, P, dev))
        if out is None:                                     # reused by every later batch of this shape
            out = self._bufs[(B, P, dev)] = (
                torch.empty((NUM_THRESHOLDS, C1, B * P), dtype=torch.float32, device=dev),
                torch.empty((NUM_THRESHOLDS, C1, B * P), dtype=torch.bool, device=dev),
                torch.empty((C1, 4, B * P), dtype=torch.bool, device=dev), torch.empty((C1, 4), dtype=torch.int64, device=dev))
        od = detect.detect_od_map(*(det[k] for k in DETECTION_KEYS), data["boxes"].reshape(B, N, 4).float().contiguous(),
                               data["classes"].reshape(B, N).contiguous(), data["active"].reshape(B, N).contiguous(),
                               data["video"].shape[-2:], self.num_classes, self.per_class, T=NUM_THRESHOLDS, out=out)
        return self.update_od(od)

    def tensors(self):
        raise RuntimeError("StreamingDetectionEvaluator keeps no per-batch tensors: only the histograms (state())")

    def state(self):
        """(hist_tp, hist_seen, anno_total) as accumulated here; None before the first update."""
        return self._state

    def aggregate(self, device=None):
        import torch.distributed as distrib
        ranks = distrib.get_world_size() if distrib.is_available() and distrib.is_initialized() else 1
        if self._state is None:
            if ranks == 1:
                raise RuntimeError("StreamingDetectionEvaluator: no update yet")
            self._state = detect.ap_hist_state(NUM_THRESHOLDS, self.num_classes + 1, "cpu" if device is None else device)
        state = self._state
        if ranks > 1:                                       # the local state stays what this rank saw
            state = tuple(t.clone() for t in state)
            for t in state:
                distrib.all_reduce(t, op=distrib.ReduceOp.SUM)
        ap, ap101, pr, score, totals = (t.cpu() for t in detect.ap_hist_finalize(state))
        anno = state[2].cpu()
        print("Number of annos for each class and size category is:")
        print(anno)
        res = _ap_tables(ap)
        res["coco"] = _ap_tables(ap101)
        res["pr_curve"] = {"precision": pr, "score": score,
                           "recall": torch.arange(101, dtype=torch.float64) / 100}
        res["operating_point"] = _operating_point(totals[0, :, 0, 1], totals[0, :, 0, 0], anno[:, 0], 0)
        return res
