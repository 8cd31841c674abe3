"""AP bookkeeping over detection rows (fod_detect_od_map, include/fod_ext.h): a numpy float32 restatement of the
definition, written from the header's text with its loops in the style of oracle/od_map.py, and the cases the CPU form,
the kernel and the public surface are held against.  It shares no helper with the package.  Every operation of the
restatement is explicitly np.float32 and rounded once, so equality of every output byte is the right comparison: no
tolerance appears anywhere but in the hand example's AP (the 1e-5 in the precision's denominator).

A case is a dict: name, the five row tensors (scores f32 [B,K], labels i32 [B,K], boxes f32 [B,K,4], query i32 [B,K],
count i32 [B]), anno_boxes f32 [B,N,4], anno_classes i64 [B,N], anno_active i64 [B,N], imsize, C, per_class, T and
want = the four outputs of the restatement (confs f32, is_positive u8, size_categories u8, num_annos i64) for
P = min(per_class, K).  Cases of group 1 also carry what they were made from: logits f32 [B,M,C], cxcywh f32 [B,M,4],
dense f32 [B,M,C+1] (sigmoid scores, the last column their maximum) and px f32 [B,M,4].

Kept from the reference's IoU, and visible in the edge cases: with the 1e-7 smoothing two ZERO-AREA boxes have IoU
(0 + 1e-7) / (0 + 1e-7) = 1 wherever they lie, so a zero-area row claims a free zero-area annotation at every threshold."""
import numpy as np

import nms_cases as NC

F = np.float32
ROWS = ("scores", "labels", "boxes", "query", "count")
ANNOS = ("anno_boxes", "anno_classes", "anno_active")
OUTS = ("confs", "is_positive", "size_categories", "num_annos")
IMSIZE = (96, 128)


# ---- the definition --------------------------------------------------------------------------------------------------
def _flags(box, finite, s0, s1):
    """[all, small, medium, large] of one box from its UNCLAMPED area; a non-finite box is (1, 0, 0, 0)."""
    if not finite:
        return np.array([1, 0, 0, 0], np.uint8)
    area = (box[2] - box[0]) * (box[3] - box[1])
    assert area.dtype == F
    return np.array([1, area <= s0, (s0 < area) and (area <= s1), s1 < area], np.uint8)


def _iou_row(p, ab):
    """One row's box against all annotation boxes [N,4]: fod_od_map's IoU, float32, every operation rounded once."""
    zero, eps = F(0), F(1e-7)
    area_p = np.maximum(p[2] - p[0], zero) * np.maximum(p[3] - p[1], zero)
    area_a = np.maximum(ab[:, 2] - ab[:, 0], zero) * np.maximum(ab[:, 3] - ab[:, 1], zero)
    inter = np.maximum(np.minimum(p[2], ab[:, 2]) - np.maximum(p[0], ab[:, 0]), zero) * \
        np.maximum(np.minimum(p[3], ab[:, 3]) - np.maximum(p[1], ab[:, 1]), zero)
    iou = (inter + eps) / (((area_p + area_a) - inter) + eps)
    assert iou.dtype == F
    return iou


def restate(scores, labels, boxes, query, count, anno_boxes, anno_classes, anno_active, imsize, C, P, T):
    """-> confs f32 [T,C1,B*P], is_positive u8 [T,C1,B*P], size_categories u8 [C1,4,B*P], num_annos i64 [C1,4]."""
    assert scores.dtype == boxes.dtype == anno_boxes.dtype == F and labels.dtype == query.dtype == count.dtype == np.int32
    assert anno_classes.dtype == anno_active.dtype == np.int64
    (B, K), N, C1 = scores.shape, anno_boxes.shape[1], C + 1
    assert 1 <= P <= K
    H, W = imsize
    s0, s1 = F((1 / 24) * (1 / 64) * float(H) * float(W)), F((1 / 4) * (1 / 12) * float(H) * float(W))
    confs = np.zeros((T, C1, B * P), F)
    is_pos = np.zeros((T, C1, B * P), np.uint8)
    sizes = np.zeros((C1, 4, B * P), np.uint8)
    num_annos = np.zeros((C1, 4), np.int64)
    for b in range(B):
        n = min(max(int(count[b]), 0), K)                   # rows at or beyond n are never read
        a_finite = np.isfinite(anno_boxes[b]).all(axis=1)
        ab = np.where(a_finite[:, None], anno_boxes[b], F(0))
        for c in range(C1):
            counted = [a for a in range(N) if anno_active[b, a] == 1 and (c == C or anno_classes[b, a] == c)]
            for a in counted:
                num_annos[c] += _flags(anno_boxes[b, a], a_finite[a], s0, s1)
            if c < C:
                cand = [j for j in range(n) if labels[b, j] == c]
            else:
                cand = [j for j in range(n) if not any(query[b, i] == query[b, j] for i in range(j))]
            cand = cand[:P]
            finite = [bool(np.isfinite(boxes[b, j]).all()) for j in cand]
            with np.errstate(all="ignore"):
                iou = [_iou_row(boxes[b, j], ab) if f else None for j, f in zip(cand, finite)]
            for k, j in enumerate(cand):
                confs[:, c, b * P + k] = scores[b, j]
                sizes[c, :, b * P + k] = _flags(boxes[b, j], finite[k], s0, s1)
            for t in range(T):
                thr = F(0.5 + t * 0.05)
                free = np.zeros(N, bool)
                free[[a for a in counted if a_finite[a]]] = True
                for k in range(len(cand)):
                    if not finite[k]:
                        continue
                    best, best_a = F(0), None
                    for a in range(N):
                        v = iou[k][a] if free[a] else F(0)
                        if best_a is None or v > best:      # ties go to the lowest index
                            best, best_a = (v if v == v else F(0)), a
                    if best >= thr:
                        is_pos[t, c, b * P + k] = 1
                        free[best_a] = False
    return confs, is_pos, sizes, num_annos


def _case(name, rows, annos, C, per_class=50, T=10, imsize=IMSIZE, **extra):
    scores, labels, boxes, query, count = rows
    c = dict(name=name, scores=np.ascontiguousarray(scores, dtype=F), labels=np.ascontiguousarray(labels, dtype=np.int32),
             boxes=np.ascontiguousarray(boxes, dtype=F), query=np.ascontiguousarray(query, dtype=np.int32),
             count=np.ascontiguousarray(count, dtype=np.int32), anno_boxes=np.ascontiguousarray(annos[0], dtype=F),
             anno_classes=np.ascontiguousarray(annos[1], dtype=np.int64),
             anno_active=np.ascontiguousarray(annos[2], dtype=np.int64), imsize=imsize, C=C, per_class=per_class, T=T, **extra)
    c["P"] = min(per_class, c["scores"].shape[1])
    c["want"] = restate(*(c[k] for k in ROWS + ANNOS), imsize, C, c["P"], T)
    return c


def slots(case, c, b=None):
    """(filled, padding) slot counts of class c (over all samples, or of sample b)."""
    col = case["want"][2][c, 0]
    if b is not None:
        col = col[b * case["P"]:(b + 1) * case["P"]]
    return int(col.sum()), int(col.size - col.sum())


# ---- random material ---------------------------------------------------------------------------------------------------
def _material(B, M, C, N, seed):
    """Logits randn * 2 with one exact tie, integer-pixel boxes (jittered copies of annotations or random), annotations
    with holes in `active`."""
    rng = np.random.RandomState(seed)
    H, W = IMSIZE
    x0, y0 = rng.randint(0, W - 24, size=(B, N)), rng.randint(0, H - 24, size=(B, N))
    w, h = rng.randint(2, 60, size=(B, N)), rng.randint(2, 50, size=(B, N))
    ab = np.stack([x0, y0, np.minimum(x0 + w, W), np.minimum(y0 + h, H)], axis=2).astype(F)
    ac = rng.randint(0, C, size=(B, N)).astype(np.int64)
    aa = (rng.uniform(size=(B, N)) < 0.75).astype(np.int64)
    aa[:, 0] = 1
    px = np.zeros((B, M, 4), F)
    for b in range(B):
        for m in range(M):
            if rng.uniform() < 0.7:
                src = ab[b, rng.randint(0, N)]
                jit = rng.randint(-3, 4, size=4) if rng.uniform() < 0.7 else np.zeros(4, int)
                box = src + jit
            else:
                bx, by = rng.randint(0, W - 10), rng.randint(0, H - 10)
                box = np.array([bx, by, bx + rng.randint(2, 50), by + rng.randint(2, 40)])
            box = np.array([max(box[0], 0), max(box[1], 0), min(box[2], W), min(box[3], H)], F)
            if box[2] <= box[0]:
                box[2] = box[0] + 1
            if box[3] <= box[1]:
                box[3] = box[1] + 1
            px[b, m] = box
    logits = (rng.randn(B, M, C) * 2).astype(F)
    logits[0, 1, 0] = logits[0, 0, 0] = float(logits[0].max()) + 0.5        # the tie: the two best scores of sample 0
    sig = (F(1) / (F(1) + np.exp(-logits.astype(np.float64)))).astype(F)
    dense = np.concatenate([sig, sig.max(axis=2, keepdims=True)], axis=2)
    cxcywh = np.stack([(px[..., 0] + px[..., 2]) * F(0.5) / F(W), (px[..., 1] + px[..., 3]) * F(0.5) / F(H),
                       (px[..., 2] - px[..., 0]) / F(W), (px[..., 3] - px[..., 1]) / F(H)], axis=2).astype(F)
    return dict(logits=logits, cxcywh=cxcywh, dense=dense, px=px), (ab, ac, aa)


def _select(dense, px, K, per_query=False, thr=0.0):
    """The K best (query, class) pairs of each sample -- per_query: of the queries, each with its best class -- best first,
    ties by flat index: the five row tensors, padded as fod_detect_select pads."""
    B, M, C1 = dense.shape
    C = C1 - 1
    out = (np.zeros((B, K), F), np.full((B, K), -1, np.int32), np.zeros((B, K, 4), F), np.full((B, K), -1, np.int32),
           np.zeros((B,), np.int32))
    for b in range(B):
        if per_query:
            pairs = [(m, int(dense[b, m, :C].argmax())) for m in range(M)]
        else:
            pairs = [(m, c) for m in range(M) for c in range(C)]
        pairs = [p for p in pairs if dense[b, p[0], p[1]] >= F(thr)]
        order = sorted(range(len(pairs)), key=lambda i: -float(dense[b, pairs[i][0], pairs[i][1]]))[:K]     # (stable)
        for r, i in enumerate(order):
            m, c = pairs[i]
            out[0][b, r], out[1][b, r], out[2][b, r], out[3][b, r] = dense[b, m, c], c, px[b, m], m
        out[4][b] = len(order)
    return out


def _check_random(c):
    """No random case is vacuous: positives and negatives at t = 0, and a decision that the threshold changes."""
    pos, filled = c["want"][1], c["want"][2][:, 0] == 1
    assert (pos[0][filled] == 1).any() and (pos[0][filled] == 0).any(), c["name"]
    assert (pos[0] != pos[c["T"] - 1]).any(), c["name"]
    return c


GROUP1_SIZES = ((2, 40, 5, 12), (2, 60, 8, 20), (1, 7, 3, 4), (3, 50, 4, 9))


def all_pairs():
    """Group 1: every pair selected, nothing cut: K = M * C, per_class = min(50, M)."""
    cases = []
    for k, (B, M, C, N) in enumerate(GROUP1_SIZES):
        mat, annos = _material(B, M, C, N, seed=300 + k)
        rows = _select(mat["dense"], mat["px"], M * C)
        assert rows[0][0, 0] == rows[0][0, 1] and (rows[4] == M * C).all()                 # the forced tie leads
        cases.append(_check_random(_case(f"all-pairs-B{B}-M{M}-C{C}-N{N}", rows, annos, C, per_class=min(50, M), **mat)))
    return cases


def cuts():
    """Group 2: K well below M * C, per_class below a class's row count, a class without rows, count 0 / > K / < 0."""
    B, M, C, N = 3, 40, 4, 10
    mat, annos = _material(B, M, C, N, seed=411)
    K = 48
    rows = _select(mat["dense"], mat["px"], K)
    cases = [_check_random(_case("cut-K48-of-160", rows, annos, C, per_class=50)),
             _check_random(_case("cut-per-class-6", rows, annos, C, per_class=6))]
    assert max(int((rows[1][b] == k).sum()) for b in range(B) for k in range(C)) > 6         # candidates beyond P exist
    # a class with no rows: class 2's rows leave, the rest closes up
    gone = [np.zeros_like(t) for t in rows]
    for b in range(B):
        keep = np.nonzero(rows[1][b] != 2)[0]
        for g, t in zip(gone[:4], rows[:4]):
            g[b, :keep.size] = t[b, keep]
        gone[4][b] = keep.size
    cases.append(_check_random(_case("cut-class-2-absent", gone, annos, C, per_class=8)))
    assert slots(cases[-1], 2) == (0, B * 8) and int(cases[-1]["want"][3][2, 0]) > 0
    for name, count in (("cut-count-0-in-the-middle", [K, 0, 5]), ("cut-count-clamped", [K + 9, -3, 2 ** 31 - 1])):
        r = rows[:4] + (np.asarray(count, np.int32),)
        cases.append(_check_random(_case(name, r, annos, C, per_class=6)))
    assert slots(cases[-2], C, b=1) == (0, 6) and slots(cases[-1], C, b=1) == (0, 6)
    inside = _case("inside", rows[:4] + (np.asarray([K, 0, K], np.int32),), annos, C, per_class=6)
    assert all(a.tobytes() == w.tobytes() for a, w in zip(cases[-1]["want"], inside["want"]))
    # the group has padding slots and candidates beyond P
    assert any(slots(k, cc)[1] > 0 for k in cases for cc in range(C + 1))
    return cases


def after_nms():
    """Group 3: the rows fod_detect_nms leaves at 0.5; the generic class sees the first surviving row of every query."""
    B, M, C, N = 2, 30, 4, 8
    mat, annos = _material(B, M, C, N, seed=523)
    rows = _select(mat["dense"], mat["px"], M * C)
    cases = []
    for agnostic in (False, True):
        kept = NC.restate(*rows, 0.5, agnostic)[:5]
        assert all(0 < int(kept[4][b]) < M * C for b in range(B))
        cases.append(_check_random(_case(f"after-nms-0.5{'-agnostic' if agnostic else ''}", kept, annos, C, per_class=50)))
        queries = kept[3][0, :int(kept[4][0])].tolist()
        assert slots(cases[-1], C, b=0)[0] == len(set(queries)) <= M
        assert agnostic or len(set(queries)) < len(queries)          # class-aware: a query survives under several classes
    return cases


def per_query():
    """Group 4: one row per query: the generic class sees every row."""
    B, M, C, N = 2, 45, 5, 10
    mat, annos = _material(B, M, C, N, seed=631)
    rows = _select(mat["dense"], mat["px"], M, per_query=True)
    c = _check_random(_case("per-query", rows, annos, C, per_class=50))
    assert slots(c, C) == (B * M, 0)
    half = _check_random(_case("per-query-K20", _select(mat["dense"], mat["px"], 20, per_query=True), annos, C, per_class=50))
    return [c, half]


# ---- edges -------------------------------------------------------------------------------------------------------------
def _rows(boxes, labels, query=None, count=None):
    """One sample: descending scores, query = row unless given."""
    boxes = np.asarray(boxes, F)[None]
    K = boxes.shape[1]
    scores = (F(0.99) - np.arange(K, dtype=F) * F(0.0009))[None].astype(F)
    query = np.arange(K) if query is None else query
    return (scores, np.asarray(labels, np.int32)[None], boxes, np.asarray(query, np.int32)[None],
            np.asarray([K if count is None else count], np.int32))


def _annos(boxes, classes, active=None):
    boxes = np.asarray(boxes, F)[None]
    N = boxes.shape[1]
    return boxes, np.asarray(classes, np.int64)[None], (np.ones((1, N), np.int64) if active is None else np.asarray(active, np.int64)[None])


def _fillers(K, y=70.0):
    r = np.arange(K, dtype=F)
    return np.stack([r % 60 * 2, y + r // 60, r % 60 * 2 + 1, y + r // 60 + 1], axis=1).astype(F)


def edges():
    nan, inf = float("nan"), float("inf")
    cases = []
    # non-finite corners on both sides: row 1 (NaN) would otherwise see row 0's annotation through min / max that drop
    # the NaN; annotation 2 (inf) is active and counted, and never claimed
    rows = _rows([[10, 10, 30, 30], [10, 10, nan, 30], [40, 40, 60, 60], [-inf, 0, 5, 5], [70, 10, 90, 30]], [0, 0, 0, 0, 0])
    annos = _annos([[10, 10, 30, 30], [40, 40, 60, 60], [70, 10, inf, 30], [nan, nan, nan, nan]], [0, 0, 0, 0], [1, 1, 1, 1])
    c = _case("non-finite", rows, annos, 1)
    assert c["want"][1][0, 0].tolist()[:5] == [1, 0, 1, 0, 0] and c["want"][3][0].tolist() == [4, 0, 0, 2]
    assert c["want"][2][0, :, 1].tolist() == [1, 0, 0, 0] and c["want"][0][0, 0, 1] == rows[0][0, 1]
    cases.append(c)
    # zero-area boxes: IoU 1 with each other under the smoothing, wherever they lie (the header of this file)
    rows = _rows([[5, 5, 5, 9], [20, 20, 30, 20], [50, 50, 60, 60]], [0, 0, 0])
    annos = _annos([[80, 80, 80, 85], [50, 50, 60, 60], [1, 1, 1, 1]], [0, 0, 0])
    c = _case("zero-area", rows, annos, 1)
    assert (c["want"][1][:, 0, :3] == 1).all()
    cases.append(c)
    # an IoU exactly at a threshold: inter 2, union 4 -> (2 + 1e-7) / (4 + 1e-7) rounds to 0.5: positive at t = 0 only
    rows = _rows([[0, 0, 2, 2], [10, 0, 12, 2]], [0, 0])
    annos = _annos([[0, 0, 2, 1], [10, 0, 12, 2]], [0, 0])
    c = _case("iou-at-threshold", rows, annos, 1)
    assert c["want"][1][:, 0, 0].tolist() == [1] + [0] * 9 and (c["want"][1][:, 0, 1] == 1).all()
    cases.append(c)
    # two annotations tied in IoU: the lower index goes first, the second row takes the other, the third finds none
    rows = _rows([[10, 10, 30, 30]] * 3, [0, 0, 0])
    annos = _annos([[50, 50, 60, 60], [10, 10, 30, 30], [10, 10, 30, 30]], [0, 0, 0])
    c = _case("tied-annotations", rows, annos, 1)
    assert (c["want"][1][:, 0, :3] == np.array([1, 1, 0])).all()
    cases.append(c)
    # extents: N = 1, N = 1024, K = 1024, with T = 10, 1, 16
    rng = np.random.RandomState(7)
    for T in (10, 1, 16):
        rows = _rows([[10, 10, 30, 30], [11, 10, 30, 30], [50, 50, 60, 60]], [0, 1, 0])
        cases.append(_case(f"N1-T{T}", rows, _annos([[10, 10, 30, 30]], [0]), 2, T=T))
        N = 1024
        ab = _fillers(N)
        ab[1023], ab[64], ab[501] = (10, 10, 30, 30), (40, 40, 60, 62), (11, 10, 30, 30)
        aa = np.ones(N, np.int64)
        aa[3::7] = 0
        rows = _rows([[10, 10, 30, 30], [10, 10, 30, 30], [40, 40, 60, 60], [0, 70, 1, 71], [5, 5, 8, 8]], [0, 1, 0, 1, 0])
        c = _case(f"N1024-T{T}", rows, _annos(ab, rng.randint(0, 2, size=N), aa), 2, T=T)
        assert aa[[1023, 64, 501]].all() and c["want"][1][0, 2, :2].tolist() == [1, 1]     # generic: 1023, then 501 (IoU 0.95)
        cases.append(c)
        K = 1024
        bx = _fillers(K)
        bx[0], bx[700], bx[1023] = (10, 10, 30, 30), (10, 10, 30, 31), (40, 40, 60, 60)
        lab = rng.randint(0, 2, size=K)
        lab[[0, 700, 1023]] = (0, 0, 1)
        rows = _rows(bx, lab, query=rng.randint(0, 300, size=K))
        annos = _annos([[10, 10, 30, 30], [40, 40, 60, 60], [0, 70, 1, 71], [10, 10, 30, 31]], [0, 1, 0, 0])
        c = _case(f"K1024-T{T}", rows, annos, 2, per_class=1024 if T == 10 else 600, T=T)
        assert c["want"][1][0, 0].sum() >= 2 and c["want"][1][0, 1].sum() >= 1      # rows 0, 700 and 1023 find theirs
        cases.append(c)
    # K = 65: the wave boundary of the compaction, P = 64 and 65, the last row a positive one
    bx = _fillers(65)
    bx[64], bx[63] = (10, 10, 30, 30), (40, 40, 60, 60)
    annos = _annos([[10, 10, 30, 30], [40, 40, 60, 60]], [0, 0])
    for P in (64, 65):
        c = _case(f"K65-P{P}", _rows(bx, [0] * 65), annos, 1, per_class=P)
        assert c["want"][1][0, 0].sum() == c["want"][1][0, 1].sum() == (1 if P == 64 else 2)
        cases.append(c)
    return cases


# ---- the hand example -----------------------------------------------------------------------------------------------------
def hand():
    """One class, two annotations; rows (0.9, a0), (0.8, a0 shifted by a pixel), (0.7, a1).  Without suppression the
    ranking is TP FP TP: AP50 = (1 + 2/3) / 2; after detect_nms(0.5) row 1 is gone: TP TP, AP50 = 1."""
    a0, a1 = [10, 10, 30, 30], [50, 50, 70, 70]
    annos = _annos([a0, a1], [0, 0])
    rows = (np.array([[0.9, 0.8, 0.7]], F), np.zeros((1, 3), np.int32), np.array([[a0, [11, 10, 31, 30], a1]], F),
            np.array([[4, 9, 2]], np.int32), np.array([3], np.int32))
    plain = _case("hand-plain", rows, annos, 1)
    kept = NC.restate(*rows, 0.5, False)
    assert kept[4].tolist() == [2] and kept[5][0].tolist() == [0, 2, -1]
    nms = _case("hand-nms-0.5", kept[:5], annos, 1)
    assert plain["want"][1][0, 0].tolist()[:3] == [1, 0, 1] and nms["want"][1][0, 0].tolist()[:3] == [1, 1, 0]
    assert slots(plain, 0) == (3, 0) and slots(nms, 0) == (2, 1)
    return plain, nms


HAND_AP50 = ((1 + 2 / 3) / 2, 1.0)


def all_cases():
    return all_pairs() + cuts() + after_nms() + per_query() + edges() + list(hand())
