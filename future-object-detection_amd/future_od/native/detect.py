"""Operations on DETECTION ROWS, the five tensors fod_detect_select writes, and the dense bookkeeping they replace:
selection, NMS, AP bookkeeping, tracker, streaming AP.  This module holds the kernels' wrappers TOGETHER WITH the host
definitions of the same contracts (include/fod.h, include/fod_ext.h): on CPU tensors a wrapper runs the plain per-sample
form, byte for byte what the kernel writes; on device tensors it checks the operands (a wrong extent would be an
out-of-bounds access on the GPU) and launches through `ops.call` on `ops.stream()`, both looked up at every launch (tools
count launches and tests stub them by replacing those two)."""
import math

import torch

from . import lib as L
from . import ops
from .ops import _chk, ptr

ROWS_MAX = 1024                                          # rows K, annotations N, track slots S (csrc/det_rows.h)
_F, _I, _L, _ZERO = torch.float32, torch.int32, torch.int64, torch.zeros((), dtype=torch.float32)


def _expect(who, tensors, specs, dev, what=""):
    """Every tensor is contiguous, on `dev`, and of its spec's (name, dtype or tuple of dtypes, shape); None is skipped."""
    for t, (name, dtypes, shape) in zip(tensors, specs):
        dtypes = dtypes if isinstance(dtypes, tuple) else (dtypes,)
        if t is not None and (tuple(t.shape) != shape or t.dtype not in dtypes or t.device != dev or not t.is_contiguous()):
            raise L.FodError(f"{who}: contiguous {what}{name} {dtypes[0]} {list(shape)} on {dev} expected, got {t.dtype} "
                             f"{tuple(t.shape)} strides {t.stride()} on {t.device}")


def _empty(specs, dev):
    return tuple(torch.empty(shape, dtype=d[0] if isinstance(d, tuple) else d, device=dev) for _name, d, shape in specs)


def _row_specs(B, K):
    return (("scores", _F, (B, K)), ("labels", _I, (B, K)), ("boxes", _F, (B, K, 4)), ("query", _I, (B, K)),
            ("count", _I, (B,)))


def _od_specs(T, C1, slots, flag=(torch.bool, torch.uint8)):
    return (("confs", _F, (T, C1, slots)), ("is_positive", flag, (T, C1, slots)), ("size_categories", flag, (C1, 4, slots)),
            ("num_annos", _L, (C1, 4)))


# ---- what the host definitions share: f32 tensor operations, each rounded once, in the order the headers write them -----
_f32 = lambda v: torch.tensor(v, dtype=_F)
_row_count = lambda count, b, K: min(max(int(count[b]), 0), K)          # rows at or beyond it are never read
_finite_rows = lambda bx: torch.isfinite(bx).all(dim=1)


def _clamped_area(bx):
    return torch.maximum(bx[..., 2] - bx[..., 0], _ZERO) * torch.maximum(bx[..., 3] - bx[..., 1], _ZERO)


def _intersection(a, q):                                 # boxes [..., 4] that broadcast against each other
    return torch.maximum(torch.minimum(a[..., 2], q[..., 2]) - torch.maximum(a[..., 0], q[..., 0]), _ZERO) * \
        torch.maximum(torch.minimum(a[..., 3], q[..., 3]) - torch.maximum(a[..., 1], q[..., 1]), _ZERO)


def _store(out, res):
    """A host definition's results into the caller's tensors (None: not wanted), all read before any is written."""
    for o, r in zip(out, res):
        if o is not None:
            o.copy_(r)
    return tuple(out)


def post_proc(logits, boxes, img_h, img_w):
    _chk(logits, "logits", torch.float32); _chk(boxes, "boxes", torch.float32)
    Cc = logits.shape[-1]
    R = logits.numel() // Cc
    assert boxes.numel() == R * 4
    scores = torch.empty(logits.shape[:-1] + (Cc + 1,), dtype=torch.float32, device=logits.device)
    boxes_px = torch.empty_like(boxes)
    ops.call("fod_post_proc", ptr(logits), ptr(boxes), ptr(scores), ptr(boxes_px), R, Cc, float(img_h),
             float(img_w), ops.stream())
    return scores, boxes_px


def detect_select(logits, boxes, img_h, img_w, top_k=100, score_threshold=0.0, per_query=False, box_map=None, out=None):
    """logits f32 [B,M,C], boxes f32 [B,M,4] cxcywh in (0,1) -> (scores f32 [B,K], labels i32 [B,K], boxes f32 [B,K,4]
    xyxy pixels, query i32 [B,K], count i32 [B]): the K best candidates of each sample, one launch (fod_detect_select in
    include/fod.h has the exact semantics).  `box_map` f32 [B,4] = (sx, sy, ox, oy) moves the boxes into another frame.
    `out`: five tensors of those shapes to write into instead of new ones."""
    _chk(logits, "logits", torch.float32); _chk(boxes, "boxes", torch.float32)
    if logits.dim() != 3 or boxes.shape != logits.shape[:2] + (4,):
        raise L.FodError(f"detect_select: logits [B,M,C] and boxes [B,M,4] expected, got {tuple(logits.shape)} and "
                         f"{tuple(boxes.shape)}")
    B, M, Cc = logits.shape
    K, dev = int(top_k), logits.device
    _expect("detect_select", (box_map,), (("box_map", torch.float32, (B, 4)),), dev)
    if out is None:
        out = _empty(_row_specs(B, max(K, 0)), dev)
    scores, labels, boxes_px, query, count = out
    _expect("detect_select", out, _row_specs(B, K), dev, "out ")
    ops.call("fod_detect_select", ptr(logits), ptr(boxes), ptr(box_map), B, M, Cc, K, float(score_threshold),
             int(bool(per_query)), float(img_h), float(img_w), ptr(scores), ptr(labels), ptr(query), ptr(boxes_px),
             ptr(count), ops.stream())
    return scores, labels, boxes_px, query, count


def _detect_nms_cpu(scores, labels, boxes, query, count, thr, class_agnostic):
    """The definition of fod_detect_nms (include/fod_ext.h) on host tensors, sample by sample: f32 tensor operations,
    each rounded once; a row's test against all later rows is one vector expression."""
    B, K = scores.shape
    out = (torch.zeros_like(scores), torch.full_like(labels, -1), torch.zeros_like(boxes), torch.full_like(query, -1),
           torch.zeros_like(count), torch.full_like(labels, -1))
    thr = _f32(thr)
    for b in range(B):
        n = _row_count(count, b, K)
        bx, lb = boxes[b, :n], labels[b, :n]
        finite, area = _finite_rows(bx), _clamped_area(bx)
        gone = torch.zeros(n, dtype=torch.bool)
        for i in range(n):
            if gone[i] or not finite[i]:
                continue
            inter = _intersection(bx[i], bx[i + 1:])
            uni = (area[i] + area[i + 1:]) - inter
            hit = (inter > thr * uni) & finite[i + 1:]
            if not class_agnostic:
                hit &= lb[i + 1:] == lb[i]
            gone[i + 1:] |= hit
        src = torch.nonzero(~gone).flatten()
        m = src.numel()
        for o, t in zip(out[:4], (scores, labels, boxes, query)):
            o[b, :m] = t[b, src]
        out[4][b] = m
        out[5][b, :m] = src.to(torch.int32)
    return out


def detect_nms(scores, labels, boxes, query, count, iou_threshold=0.5, class_agnostic=False, out=None):
    """Greedy hard NMS over the five tensors of detect_select, one launch (fod_detect_nms in include/fod_ext.h has the
    exact semantics): per sample the rows below `count` in row order, a row dropped iff a kept earlier row of its class
    (`class_agnostic`: of any class) has inter > iou_threshold * union with it.
    -> (scores, labels, boxes, query, count, source): the survivors at the front, padding behind them, `source` i32 [B,K]
    the input row of every output row (-1 for padding).  `out`: six tensors of those shapes to write into instead of new
    ones; the first five may be the inputs themselves (in place).  CPU tensors run the plain per-sample form of the same
    definition (same bits); device tensors run the kernel."""
    if scores.dim() != 2:
        raise L.FodError(f"detect_nms: scores [B,K] expected, got {tuple(scores.shape)}")
    (B, K), dev = scores.shape, scores.device
    specs = _row_specs(B, K)
    _expect("detect_nms", (scores, labels, boxes, query, count), specs, dev)
    thr = float(iou_threshold)
    if not (math.isfinite(thr) and 0.0 <= thr <= 1.0):
        raise L.FodError(f"detect_nms: iou_threshold={thr} is outside [0, 1]")
    if B < 1 or not 1 <= K <= ROWS_MAX:
        raise L.FodError(f"detect_nms: B={B} (at least 1) and K={K} (1..{ROWS_MAX}) expected")
    if out is None:
        out = tuple(torch.empty_like(t) for t in (scores, labels, boxes, query, count, labels))
    if len(out) != 6:
        raise L.FodError("detect_nms: out is (scores, labels, boxes, query, count, source)")
    _expect("detect_nms", out, specs + (("source", torch.int32, (B, K)),), dev, "out ")
    if not scores.is_cuda:
        return _store(out, _detect_nms_cpu(scores, labels, boxes, query, count, thr, bool(class_agnostic)))
    ops.call("fod_detect_nms", ptr(scores), ptr(labels), ptr(boxes), ptr(query), ptr(count), B, K, thr,
             int(bool(class_agnostic)), *(ptr(o) for o in out), ops.stream())
    return tuple(out)


def od_map(scores, boxes_px, anno_boxes, anno_classes, anno_active, imsize, T=10):
    _chk(scores, "scores", torch.float32); _chk(boxes_px, "boxes", torch.float32)
    _chk(anno_boxes, "anno_boxes", torch.float32)
    _chk(anno_classes, "anno_classes", torch.int64); _chk(anno_active, "anno_active", torch.int64)
    B, M, C1 = scores.shape
    N = anno_classes.shape[1]
    assert boxes_px.shape == (B, M, 4) and anno_boxes.shape == (B, N, 4) and anno_active.shape == (B, N)
    K = min(50, M)
    out = _empty(_od_specs(T, C1, B * K), scores.device)              # confs, is_positive, size_categories, num_annos
    ops.call("fod_od_map", ptr(scores), ptr(boxes_px), ptr(anno_boxes), ptr(anno_classes), ptr(anno_active),
             *(ptr(o) for o in out), B, M, C1, N, T, float(imsize[0]), float(imsize[1]), ops.stream())
    return out


def _detect_od_map_cpu(scores, labels, boxes, query, count, anno_boxes, anno_classes, anno_active, H, W, C, P, T):
    """The definition of fod_detect_od_map (include/fod_ext.h) on host tensors, sample by sample: f32 tensor operations,
    each rounded once; a sample's IoU table is one vector expression, the greedy walk is a loop."""
    (B, K), N, C1 = scores.shape, anno_boxes.shape[1], C + 1
    zero, eps = _ZERO, _f32(1e-7)
    s0, s1 = _f32((1.0 / 24) * (1.0 / 64) * float(H) * float(W)), _f32((1.0 / 4) * (1.0 / 12) * float(H) * float(W))
    confs = torch.zeros((T, C1, B * P), dtype=torch.float32)
    is_pos = torch.zeros((T, C1, B * P), dtype=torch.bool)
    sizes = torch.zeros((C1, 4, B * P), dtype=torch.bool)
    num_annos = torch.zeros((C1, 4), dtype=torch.int64)

    def flags(bx, finite):                               # [R,4]: column 0 always, 1..3 from the unclamped area
        area = (bx[:, 2] - bx[:, 0]) * (bx[:, 3] - bx[:, 1])
        return torch.stack([torch.ones_like(finite), finite & (area <= s0), finite & (s0 < area) & (area <= s1),
                            finite & (s1 < area)], dim=1)

    for b in range(B):
        n = _row_count(count, b, K)
        a_fin = _finite_rows(anno_boxes[b])
        a_flags = flags(anno_boxes[b], a_fin)
        ab = torch.where(a_fin[:, None], anno_boxes[b], zero)
        a_area = _clamped_area(ab)
        for c in range(C1):
            counted = (anno_active[b] == 1) & ((anno_classes[b] == c) if c < C else torch.ones(N, dtype=torch.bool))
            num_annos[c] += (counted[:, None] & a_flags).sum(dim=0)
            if c < C:
                rows = torch.nonzero(labels[b, :n] == c).flatten()[:P]
            else:
                seen, first = set(), []
                for j, q in enumerate(query[b, :n].tolist()):
                    if q not in seen:
                        seen.add(q)
                        first.append(j)
                rows = torch.tensor(first[:P], dtype=torch.int64)
            m = rows.numel()
            if m == 0:
                continue
            pb = boxes[b, rows]
            p_fin = _finite_rows(pb)
            at = slice(b * P, b * P + m)
            confs[:, c, at] = scores[b, rows]
            sizes[c, :, at] = flags(pb, p_fin).T
            inter = _intersection(pb[:, None], ab[None])
            iou = (inter + eps) / (((_clamped_area(pb)[:, None] + a_area[None]) - inter) + eps)
            iou = torch.where(iou == iou, iou, zero)       # a NaN never wins the comparison `iou > best`
            for t in range(T):
                thr = _f32(0.5 + t * 0.05)
                free = counted & a_fin
                for k in range(m):
                    if not p_fin[k]:
                        continue
                    cand = torch.where(free, iou[k], zero)
                    best = int(cand.argmax())                # the first of equal maxima: the lowest index
                    if cand[best] >= thr:
                        is_pos[t, c, b * P + k] = True
                        free[best] = False
    return confs, is_pos, sizes, num_annos


def detect_od_map(scores, labels, boxes, query, count, anno_boxes, anno_classes, anno_active, imsize, num_classes,
                  per_class=50, T=10, out=None):
    """The AP bookkeeping of `od_map` over detection ROWS, one launch (fod_detect_od_map in include/fod_ext.h has the
    exact semantics): the five tensors of detect_select / detect_nms plus the dense annotations of od_map (boxes f32
    [B,N,4], classes i64 [B,N], active i64 [B,N]) -> (confs f32 [T,C1,B*P], is_positive bool [T,C1,B*P], size_categories
    bool [C1,4,B*P], num_annos i64 [C1,4]) with C1 = num_classes + 1 and P = min(per_class, K) slots per sample and
    class.  Row order is the ranking; the generic class sees each query's first row.  `out`: four tensors of those shapes
    (bool or uint8 for the two flag tensors) to write into instead of new ones.  CPU tensors run the plain per-sample form
    of the same definition (same bytes); device tensors run the kernel."""
    if scores.dim() != 2 or anno_classes.dim() != 2:
        raise L.FodError(f"detect_od_map: scores [B,K] and anno_classes [B,N] expected, got {tuple(scores.shape)} and "
                         f"{tuple(anno_classes.shape)}")
    (B, K), N, dev = scores.shape, anno_classes.shape[1], scores.device
    _expect("detect_od_map", (scores, labels, boxes, query, count, anno_boxes, anno_classes, anno_active),
            _row_specs(B, K) + (("anno_boxes", _F, (B, N, 4)), ("anno_classes", _L, (B, N)), ("anno_active", _L, (B, N))), dev)
    C, T, per_class = int(num_classes), int(T), int(per_class)
    if B < 1 or not 1 <= K <= ROWS_MAX or not 1 <= N <= ROWS_MAX:
        raise L.FodError(f"detect_od_map: B={B} (at least 1), K={K} (1..{ROWS_MAX}) and N={N} (1..{ROWS_MAX}) expected")
    if C < 1 or per_class < 1 or not 1 <= T <= 16:
        raise L.FodError(f"detect_od_map: num_classes={C} (at least 1), per_class={per_class} (at least 1) and T={T} "
                         f"(1..16) expected")
    H, W = float(imsize[0]), float(imsize[1])
    C1, P = C + 1, min(per_class, K)
    specs = _od_specs(T, C1, B * P)
    if out is None:
        out = _empty(specs, dev)
    if len(out) != 4:
        raise L.FodError("detect_od_map: out is (confs, is_positive, size_categories, num_annos)")
    _expect("detect_od_map", out, specs, dev, "out ")
    if not scores.is_cuda:
        return _store(out, _detect_od_map_cpu(scores, labels, boxes, query, count, anno_boxes, anno_classes, anno_active,
                                              H, W, C, P, T))
    ops.call("fod_detect_od_map", ptr(scores), ptr(labels), ptr(boxes), ptr(query), ptr(count), ptr(anno_boxes),
             ptr(anno_classes), ptr(anno_active), *(ptr(o) for o in out), B, K, N, C, P, T, H, W, ops.stream())
    return tuple(out)


def _track_update_cpu(scores, labels, boxes, count, state, thr, birth, max_misses, class_agnostic, motion):
    """The definition of fod_track_update (include/fod_ext.h) on host tensors, sample by sample, the state updated in
    place: f32 tensor operations, each rounded once; a row's IoU with every slot is one vector expression."""
    tb, tv, tm, ts, next_id = state
    B, K = scores.shape
    out_track, out_hits, out_slot = torch.full_like(labels, -1), torch.zeros_like(labels), torch.full_like(labels, -1)
    thr, birth, zero = _f32(thr), _f32(birth), _ZERO
    for b in range(B):
        n = _row_count(count, b, K)
        meta, bx, lb, sc = tm[b], boxes[b, :n], labels[b, :n], scores[b, :n]
        live = meta[:, 0] >= 0
        gap = torch.where(live, meta[:, 3] + 1, torch.ones_like(meta[:, 3])).to(torch.float32)[:, None]
        pred = tb[b] + tv[b] * gap if motion else tb[b].clone()
        free_to_claim = live & _finite_rows(pred)
        pred = torch.where(free_to_claim[:, None], pred, zero)
        parea = _clamped_area(pred)
        finite = _finite_rows(bx)
        slot_row = torch.full((tb.shape[1],), -1, dtype=torch.int64)
        row_slot = torch.full((n,), -1, dtype=torch.int64)
        for j in range(n):
            if not finite[j]:
                continue
            seen = free_to_claim if class_agnostic else free_to_claim & (meta[:, 1] == lb[j])
            if not seen.any():
                continue
            inter = _intersection(bx[j], pred)
            uni = (_clamped_area(bx[j]) + parea) - inter
            iou = torch.where(uni > 0, inter / torch.where(uni > 0, uni, torch.ones_like(uni)), zero)
            iou = torch.where(seen, iou, torch.full_like(iou, -1.0))
            s = int(torch.nonzero(iou == iou.max())[0])   # the greatest IoU, ties to the lowest slot
            if inter[s] > 0 and iou[s] >= thr:
                free_to_claim = free_to_claim.clone()
                free_to_claim[s] = False
                slot_row[s], row_slot[j] = j, s
        ms = torch.nonzero(slot_row >= 0).flatten()
        mj = slot_row[ms]
        new = bx[mj]
        tv[b, ms] = (new - tb[b, ms]) / gap[ms] if motion else torch.zeros_like(new)
        tb[b, ms], ts[b, ms] = new, sc[mj]
        meta[ms, 1], meta[ms, 2], meta[ms, 3] = lb[mj], meta[ms, 2] + 1, 0
        out_track[b, mj], out_hits[b, mj], out_slot[b, mj] = meta[ms, 0], meta[ms, 2], ms.to(torch.int32)
        aged = live & (slot_row < 0)
        meta[aged, 3] += 1
        dead = aged & (meta[:, 3] > max_misses)
        meta[dead] = torch.tensor([-1, -1, 0, 0], dtype=torch.int32)
        tb[b, dead], tv[b, dead], ts[b, dead] = 0.0, 0.0, 0.0
        free = torch.nonzero(meta[:, 0] < 0).flatten()
        cand = torch.nonzero(finite & (row_slot < 0) & (sc >= birth)).flatten()
        r = min(free.numel(), cand.numel())
        free, cand = free[:r], cand[:r]
        ids = int(next_id[b]) + torch.arange(r, dtype=torch.int32)
        tb[b, free], tv[b, free], ts[b, free] = bx[cand], 0.0, sc[cand]
        meta[free, 0], meta[free, 1], meta[free, 2], meta[free, 3] = ids, lb[cand], 1, 0
        out_track[b, cand], out_hits[b, cand], out_slot[b, cand] = ids, 1, free.to(torch.int32)
        next_id[b] += r
    return out_track, out_hits, out_slot


def track_update(scores, labels, boxes, count, state, *, iou_threshold, birth_score, max_misses, class_agnostic, motion,
                 out=None):
    """One call of the tracker, one launch (fod_track_update in include/fod_ext.h has the exact semantics): the rows of
    detect_select / detect_nms (scores f32 [B,K], labels i32 [B,K], boxes f32 [B,K,4], count i32 [B]; `query` is not
    needed) claim the tracks of `state` = (boxes f32 [B,S,4], vel f32 [B,S,4], meta i32 [B,S,4] = (id, label, hits,
    misses), scores f32 [B,S], next_id i32 [B]), which is updated IN PLACE.  -> (track i32 [B,K], hits i32 [B,K], slot
    i32 [B,K]): the identity of every row (-1: none), how often it has been seen, and the slot that holds it.  `out`:
    (track, hits) or (track, hits, slot) to write into instead of new tensors; a slot of None is not written, and comes
    back as None.  CPU tensors run the plain per-sample form of the same definition (same bytes); device tensors run the
    kernel."""
    if scores.dim() != 2 or len(state) != 5 or state[0].dim() != 3:
        raise L.FodError("track_update: scores [B,K] and state = (boxes [B,S,4], vel, meta, scores, next_id) expected")
    (B, K), S, dev = scores.shape, state[0].shape[1], scores.device
    rows = _row_specs(B, K)
    _expect("track_update", (scores, labels, boxes, count) + tuple(state), rows[:3] + rows[4:] + (     # (no `query`)
        ("state boxes", _F, (B, S, 4)), ("state vel", _F, (B, S, 4)), ("state meta", _I, (B, S, 4)),
        ("state scores", _F, (B, S)), ("state next_id", _I, (B,))), dev)
    thr, birth, max_misses = float(iou_threshold), float(birth_score), int(max_misses)
    if not (math.isfinite(thr) and 0.0 <= thr <= 1.0):
        raise L.FodError(f"track_update: iou_threshold={thr} is outside [0, 1]")
    if B < 1 or not 1 <= K <= ROWS_MAX or not 1 <= S <= ROWS_MAX or max_misses < 0:
        raise L.FodError(f"track_update: B={B} (at least 1), K={K} (1..{ROWS_MAX}), S={S} (1..{ROWS_MAX}) and "
                         f"max_misses={max_misses} (not negative) expected")
    if out is None:
        out = tuple(torch.empty_like(labels) for _ in range(3))
    if len(out) == 2:
        out = tuple(out) + (None,)
    if len(out) != 3 or out[0] is None or out[1] is None:
        raise L.FodError("track_update: out is (track, hits) or (track, hits, slot)")
    _expect("track_update", out, tuple((name, torch.int32, (B, K)) for name in ("track", "hits", "slot")), dev, "out ")
    # the state is written while the detections are read: no tensor may serve twice
    ptrs = [t.data_ptr() for t in (scores, labels, boxes, count) + tuple(state) + tuple(out) if t is not None]
    if len(set(ptrs)) != len(ptrs):
        raise L.FodError("track_update: the detections, the five state tensors and the outputs must be distinct tensors")
    if not scores.is_cuda:
        return _store(out, _track_update_cpu(scores, labels, boxes, count, state, thr, birth, max_misses,
                                             bool(class_agnostic), bool(motion)))
    ops.call("fod_track_update", ptr(scores), ptr(labels), ptr(boxes), ptr(count), B, K, ptr(state[0]), ptr(state[1]),
             ptr(state[2]), ptr(state[3]), ptr(state[4]), S, thr, birth, max_misses, int(bool(class_agnostic)),
             int(bool(motion)), ptr(out[0]), ptr(out[1]), ptr(out[2]), ops.stream())
    return tuple(out)


# ------------------------------------------------------------------------------------------------ streaming AP
AP_HIST_BINS = 0x3F81                                    # bf16 patterns 0 .. 0x3F80 (1.0)
AP_HIST_POINTS = 101


def ap_hist_keys(scores):
    """The bin of every f32 score (fod_ap_hist_accum in include/fod_ext.h): 0 for NaN and s <= 0, else the score's bf16
    truncation `bits >> 16`, at most 0x3F80.  -> i64, integer arithmetic only."""
    s = scores.contiguous()
    key = (s.view(torch.int32).to(torch.int64) >> 16).clamp(max=AP_HIST_BINS - 1)
    return torch.where(s > 0, key, torch.zeros_like(key))


def ap_hist_state(T, C1, device):
    """The zeroed state of the streaming AP: (hist_tp i32 [T,C1,4,NB], hist_seen i32 [C1,4,NB], anno_total i64 [C1,4])
    with NB = 16257 score bins.  Its size does not depend on the data; states of several processes combine by adding."""
    T, C1 = int(T), int(C1)
    if not 1 <= T <= 16 or C1 < 2:
        raise L.FodError(f"ap_hist_state: T={T} (1..16) and C1={C1} (at least 2) expected")
    return (torch.zeros((T, C1, 4, AP_HIST_BINS), dtype=torch.int32, device=device),
            torch.zeros((C1, 4, AP_HIST_BINS), dtype=torch.int32, device=device),
            torch.zeros((C1, 4), dtype=torch.int64, device=device))


def _ap_hist_check_state(state, who):
    if len(state) != 3 or state[0].dim() != 4:
        raise L.FodError(f"{who}: state is (hist_tp [T,C1,4,NB], hist_seen [C1,4,NB], anno_total [C1,4])")
    T, C1, dev = state[0].shape[0], state[0].shape[1], state[0].device
    _expect(who, state, (("hist_tp", _I, (T, C1, 4, AP_HIST_BINS)), ("hist_seen", _I, (C1, 4, AP_HIST_BINS)),
                         ("anno_total", _L, (C1, 4))), dev, "state ")
    if not 1 <= T <= 16 or C1 < 2:
        raise L.FodError(f"{who}: T={T} (1..16) and C1={C1} (at least 2) expected")
    return T, C1, dev


def ap_hist_accum(od, state):
    """Fold one batch of the AP bookkeeping into the streaming state, one launch (fod_ap_hist_accum in include/fod_ext.h
    has the exact semantics): `od` = (confs f32 [T,C1,P], is_positive bool|u8 [T,C1,P], size_categories bool|u8 [C1,4,P],
    num_annos i64 [C1,4]) as `od_map` / `detect_od_map` (prepare_od_map_stuffs / prepare_od_map_detections) return them,
    `state` from `ap_hist_state`, updated IN PLACE and returned.  The bin of a slot is that of its score at t = 0; padding
    slots add nothing.  Integer sums: the state does not depend on the order of the slots or of the batches.  CPU tensors
    run the plain form of the same definition (same bytes); device tensors run the kernel."""
    T, C1, dev = _ap_hist_check_state(state, "ap_hist_accum")
    if len(od) != 4 or od[0].dim() != 3:
        raise L.FodError("ap_hist_accum: od is (confs [T,C1,P], is_positive, size_categories, num_annos)")
    P = od[0].shape[2]
    _expect("ap_hist_accum", od, _od_specs(T, C1, P), dev)
    if P < 1:
        raise L.FodError("ap_hist_accum: at least one slot expected")
    if not dev.type == "cuda":
        (confs, is_pos, sizes, num_annos), (hist_tp, hist_seen, anno_total) = od, state
        rows = (torch.arange(C1, dtype=torch.int64)[:, None] * 4) * AP_HIST_BINS + ap_hist_keys(confs[0])      # [C1,P]
        for s in range(4):
            f = sizes[:, s] != 0
            at = (rows + s * AP_HIST_BINS).flatten()
            hist_seen.view(-1).index_add_(0, at, f.flatten().to(torch.int32))
            hist_tp.view(T, -1).index_add_(1, at, ((is_pos != 0) & f[None]).reshape(T, -1).to(torch.int32))
        anno_total += num_annos
        return state
    ops.call("fod_ap_hist_accum", *(ptr(t) for t in od), T, C1, P, *(ptr(t) for t in state), ops.stream())
    return state


def _ap_hist_finalize_cpu(hist_tp, hist_seen, anno_total, T, C1):
    """The definition of fod_ap_hist_finalize on host tensors: per (class, size) row only the non-empty bins are visited
    (an empty bin changes no sum and answers no recall point); integers in i64, everything after them in f64."""
    nan = float("nan")
    ap = torch.full((T, C1, 4), nan, dtype=torch.float64)
    ap101, pr = ap.clone(), torch.full((T, C1, 4, AP_HIST_POINTS), nan, dtype=torch.float64)
    score = torch.full((T, C1, 4, AP_HIST_POINTS), nan, dtype=torch.float32)
    totals = torch.stack([hist_tp.sum(dim=3, dtype=torch.int64),
                          hist_seen.sum(dim=2, dtype=torch.int64)[None].expand(T, -1, -1)], dim=3).contiguous()
    steps = torch.arange(AP_HIST_POINTS, dtype=torch.int64)
    above = lambda x: x.flip(-1).cumsum(-1).flip(-1)                      # inclusive sums over the bins of key >= b
    for c in range(C1):
        for s in range(4):
            A = int(anno_total[c, s])
            if A <= 0:
                continue
            bins = torch.nonzero(hist_seen[c, s] > 0).flatten()          # ascending
            tp, se = hist_tp[:, c, s, bins].to(torch.int64), hist_seen[c, s, bins].to(torch.int64)
            TP, SE = above(tp), above(se)[None]
            ap[:, c, s] = (tp.double() * (TP.double() / (SE.double() + 1e-5))).sum(dim=1) / float(A)
            if not bins.numel():
                pr[:, c, s], score[:, c, s], ap101[:, c, s] = 0.0, 0.0, 0.0
                continue
            env = (TP.double() / SE.double()).cummax(dim=1).values
            # TP falls with the bin: the bins that reach recall point i are the first `reach` ones
            reach = (TP[:, None, :] * 100 >= (steps * A)[None, :, None]).sum(dim=2)            # [T,101]
            at = (reach - 1).clamp(min=0)
            edges = (bins << 16).to(torch.int32).view(torch.float32)
            pr[:, c, s] = torch.where(reach > 0, env.gather(1, at), torch.zeros((), dtype=torch.float64))
            score[:, c, s] = torch.where(reach > 0, edges[at], torch.zeros((), dtype=torch.float32))
            total = torch.zeros(T, dtype=torch.float64)
            for i in range(AP_HIST_POINTS):                               # ascending, as the contract says
                total = total + pr[:, c, s, i]
            ap101[:, c, s] = total / 101.0
    return ap, ap101, pr, score, totals


def ap_hist_finalize(state):
    """The streaming state -> (ap f64 [T,C1,4], ap101 f64 [T,C1,4], pr f64 [T,C1,4,101], pr_score f32 [T,C1,4,101],
    totals i64 [T,C1,4,2]), one launch (fod_ap_hist_finalize in include/fod_ext.h has the exact semantics): the
    reference's AP taken on score bins, COCO's 101-point interpolated AP, the precision envelope and the score's lower
    edge at recall i / 100, and (true positives, candidates) per row.  NaN where a row has no annotation.  The state is
    read only.  CPU tensors run the plain form of the same definition; device tensors run the kernel."""
    T, C1, dev = _ap_hist_check_state(state, "ap_hist_finalize")
    if not dev.type == "cuda":
        return _ap_hist_finalize_cpu(*state, T, C1)
    out = (torch.empty((T, C1, 4), dtype=torch.float64, device=dev), torch.empty((T, C1, 4), dtype=torch.float64, device=dev),
           torch.empty((T, C1, 4, AP_HIST_POINTS), dtype=torch.float64, device=dev),
           torch.empty((T, C1, 4, AP_HIST_POINTS), dtype=torch.float32, device=dev),
           torch.empty((T, C1, 4, 2), dtype=torch.int64, device=dev))
    ops.call("fod_ap_hist_finalize", ptr(state[0]), ptr(state[1]), ptr(state[2]), T, C1, *(ptr(o) for o in out), ops.stream())
    return out
