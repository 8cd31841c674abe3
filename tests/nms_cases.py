"""Duplicate suppression (fod_detect_nms, include/fod_ext.h): a numpy float32 restatement of the definition and the cases
the CPU form, the kernel and predict() are held against.  It shares no helper with the package.  Every operation of the
restatement is explicitly np.float32 and rounded once, so equality of count, source and every output byte is the right
comparison: no tolerance appears anywhere.

A case is a dict: name, the five inputs (scores f32 [B,K], labels i32 [B,K], boxes f32 [B,K,4], query i32 [B,K], count
i32 [B]), thr, agnostic, and want = the six outputs of the restatement (scores, labels, boxes, query, count, source).
Cases whose answer is known by hand assert it here, on the restatement, when the case is built."""
import numpy as np

F = np.float32
NAMES = ("scores", "labels", "boxes", "query", "count", "source")


def restate(scores, labels, boxes, query, count, thr, agnostic, pairs=None):
    """The definition, row by row: row j < n is kept iff no KEPT row i < j suppresses it.  `pairs` (a list) receives
    (b, rows i, j, decisions) for every pair that is evaluated: all kept finite rows i < j of j's class (any class when
    agnostic), without an early exit."""
    B, K = scores.shape
    out = [np.zeros((B, K), F), np.full((B, K), -1, np.int32), np.zeros((B, K, 4), F), np.full((B, K), -1, np.int32),
           np.zeros((B,), np.int32), np.full((B, K), -1, np.int32)]
    thr, zero = F(thr), F(0)
    assert boxes.dtype == F and scores.dtype == F and labels.dtype == query.dtype == count.dtype == np.int32
    for b in range(B):
        n = min(max(int(count[b]), 0), K)
        bx = boxes[b, :n]                                   # rows at or beyond n are never read
        x0, y0, x1, y1 = bx[:, 0], bx[:, 1], bx[:, 2], bx[:, 3]
        finite = np.isfinite(bx).all(axis=1)
        with np.errstate(all="ignore"):
            area = np.maximum(x1 - x0, zero) * np.maximum(y1 - y0, zero)
        is_kept = np.zeros(n, dtype=bool)
        for j in range(n):
            if finite[j]:
                same = np.ones(j, dtype=bool) if agnostic else labels[b, :j] == labels[b, j]
                i = np.nonzero(is_kept[:j] & finite[:j] & same)[0]
                with np.errstate(all="ignore"):
                    iw = np.maximum(np.minimum(x1[i], x1[j]) - np.maximum(x0[i], x0[j]), zero)
                    ih = np.maximum(np.minimum(y1[i], y1[j]) - np.maximum(y0[i], y0[j]), zero)
                    inter = iw * ih
                    uni = (area[i] + area[j]) - inter
                    hit = inter > thr * uni
                assert inter.dtype == uni.dtype == F
                if pairs is not None and i.size:
                    pairs.append((b, i, j, hit))
                if hit.any():
                    continue
            is_kept[j] = True
        kept = np.nonzero(is_kept)[0]
        m = kept.size
        for o, t in zip(out[:4], (scores, labels, boxes, query)):
            o[b, :m] = t[b, kept]
        out[4][b] = m
        out[5][b, :m] = kept
    return tuple(out)


def kept_rows(case, b=0):
    return case["want"][5][b, :int(case["want"][4][b])].tolist()


def _case(name, boxes, labels, thr, agnostic=False, count=None, kept=None):
    """boxes [B,K,4] / labels [B,K] (lists or arrays) -> a case with descending scores and distinct query numbers that
    are not the row numbers.  `kept`: per sample, the rows known by hand to survive."""
    boxes = np.asarray(boxes, dtype=F)
    labels = np.asarray(labels, dtype=np.int32)
    if boxes.ndim == 2:
        boxes, labels = boxes[None], labels[None]
    B, K = labels.shape
    scores = (F(0.99) - np.arange(B * K, dtype=F).reshape(B, K) % K * F(0.0009)).astype(F)
    query = ((np.arange(B * K, dtype=np.int64).reshape(B, K) * 7 + 3) % 1031).astype(np.int32)
    count = np.full((B,), K, np.int32) if count is None else np.asarray(count, dtype=np.int32)
    c = dict(name=name, scores=scores, labels=labels, boxes=np.ascontiguousarray(boxes), query=query, count=count,
             thr=thr, agnostic=bool(agnostic))
    c["want"] = restate(scores, labels, boxes, query, count, thr, agnostic)
    if kept is not None:
        got = [kept_rows(c, b) for b in range(B)]
        assert got == [list(k) for k in kept], (name, got)
    return c


def _fillers(K, y=500.0):
    """K boxes of 10 x 10 that touch nothing: row r at x = 20 r."""
    r = np.arange(K, dtype=F)
    return np.stack([20 * r, np.full(K, y, F), 20 * r + 10, np.full(K, y + 10, F)], axis=1).astype(F)


# ---- strict: an IoU equal to the threshold does not suppress ---------------------------------------------------------------
def strict():
    half = [[0, 0, 2, 2], [0, 0, 2, 1],                    # inter 2, union 4: IoU = 0.5 exactly -> both stay
            [100, 0, 104, 4], [100, 0, 104, 2],            # inter 8, union 16: 0.5 again
            [200, 0, 204, 4], [200, 0, 204, 3]]            # one pixel closer: 12 / 16 -> the second goes
    quarter = [[0, 0, 2, 2], [0, 0, 1, 1],                 # 1 / 4
               [100, 0, 104, 4], [100, 0, 102, 2],         # 4 / 16
               [200, 0, 204, 4], [200, 0, 203, 2]]         # 6 / 16
    lab = [0] * 6
    return [_case("strict-0.5", half, lab, 0.5, kept=[[0, 1, 2, 3, 4]]),
            _case("strict-0.25", quarter, lab, 0.25, kept=[[0, 1, 2, 3, 4]]),
            _case("strict-0.5-agnostic", half, [0, 1, 2, 3, 4, 5], 0.5, True, kept=[[0, 1, 2, 3, 4]])]


# ---- chain: A suppresses B, B would suppress C, but B is gone ------------------------------------------------------------------
def chain():
    cases = []
    for at in (0, 62, 63, 127):
        K = 130
        boxes = _fillers(K)
        for k, x in enumerate((0.0, 4.0, 8.0)):            # [0,10], [4,14], [8,18]: 6/14 > 0.4 twice, 2/18 < 0.4
            boxes[at + k] = (x, 0, x + 10, 1)
        cases.append(_case(f"chain-at-{at}", boxes, np.zeros(K), 0.4, kept=[[r for r in range(K) if r != at + 1]]))
    return cases


# ---- far: the first row reaches the last one ---------------------------------------------------------------------------------
def far():
    K = 1024
    first, mirror = _fillers(K), _fillers(K)
    first[K - 1] = first[0]
    mirror[K - 1] = mirror[K - 2]
    lab = np.zeros(K)
    return [_case("far-0-1023", first, lab, 0.5, kept=[list(range(K - 1))]),
            _case("far-1022-1023", mirror, lab, 0.5, kept=[list(range(K - 1))])]


# ---- identical ------------------------------------------------------------------------------------------------------------
def identical():
    K = 130
    boxes = np.tile(np.array([[10, 20, 50, 80]], dtype=F), (K, 1))
    return [_case("identical-one-class", boxes, np.full(K, 4), 0.5, kept=[[0]]),
            _case("identical-K-classes", boxes, np.arange(K), 0.5, kept=[list(range(K))]),
            _case("identical-K-classes-agnostic", boxes, np.arange(K), 0.5, True, kept=[[0]]),
            _case("identical-thr-1", boxes, np.full(K, 4), 1.0, kept=[list(range(K))]),     # IoU 1 > 1 is false
            _case("single-row", boxes[:1], [2], 0.5, kept=[[0]])]


# ---- disjoint: nothing is suppressed, outputs equal inputs ---------------------------------------------------------------------
def disjoint():
    K = 200
    c = _case("disjoint", _fillers(K), np.arange(K) % 3, 0.0, True, kept=[list(range(K))])
    for k, name in enumerate(NAMES[:5]):
        assert c["want"][k].tobytes() == c[name].tobytes()
    return [c]


# ---- degenerate -------------------------------------------------------------------------------------------------------------
def degenerate():
    nan, inf = float("nan"), float("inf")
    boxes = [[5, 5, 5, 9], [5, 5, 5, 9],                   # 0, 1: zero-area duplicates, both stay (0 > thr * 0 is false)
             [10, 10, 6, 6],                               # 2: inverted corners, area 0, overlaps nothing
             [6, 6, 10, 10], [6, 6, 10, 10],               # 3 stays, 4 goes (by 3)
             [6, 6, nan, 10],                              # 5: min/max that drop the NaN would see row 3's box: kept anyway
             [200, 200, nan, 210],                         # 6: ... and it suppresses nothing:
             [200, 200, 210, 210], [200, 200, 210, 210],   # 7 stays (only 6 is before it), 8 goes (by 7)
             [-inf, 300, 310, 310], [300, 300, 310, 310],  # 9, 10: an infinite corner is kept and suppresses nothing
             [6, 6, 10, inf], [nan, nan, nan, nan],        # 11, 12
             [400, 400, 410, 410], [inf, inf, inf, inf], [400, 400, 410, 410]]    # 13 stays, 14 stays, 15 goes (by 13)
    kept = [[0, 1, 2, 3, 5, 6, 7, 9, 10, 11, 12, 13, 14]]
    return [_case("degenerate", boxes, [0] * 16, 0.5, kept=kept),
            _case("degenerate-thr-0", boxes, [0] * 16, 0.0, kept=kept),
            _case("degenerate-agnostic", boxes, list(range(16)), 0.5, True, kept=kept)]


# ---- random -------------------------------------------------------------------------------------------------------------------
RANDOM_KS = (1, 2, 63, 64, 65, 128, 300, 1024)
THRESHOLDS = (0.3, 0.5, 0.7)


def _random_inputs(K, B, n_labels, seed):
    """Centres from a few clusters plus jitter, on a 1600 x 900 frame."""
    rng = np.random.RandomState(seed)
    n_clusters = max(1, K // 3)
    centres = rng.uniform([100, 100], [1500, 800], size=(B, n_clusters, 2))
    sizes = rng.uniform(30, 160, size=(B, n_clusters, 2))
    which = rng.randint(0, n_clusters, size=(B, K))
    bi = np.arange(B)[:, None]
    c = centres[bi, which] + rng.uniform(-12, 12, size=(B, K, 2))
    s = sizes[bi, which] * rng.uniform(0.8, 1.25, size=(B, K, 2))
    boxes = np.concatenate([c - s / 2, c + s / 2], axis=2).astype(F)
    labels = rng.randint(0, n_labels, size=(B, K)).astype(np.int32)
    return boxes, labels


def random():
    cases, k = [], 0
    for K in RANDOM_KS:
        for counts in ((0, 1, K), (K, K // 2, 3)):
            combos = [(THRESHOLDS[k % 3], (1, 3, 9)[(k // 2) % 3], bool(k % 2))]
            if K == 300:                                   # the default query count: every threshold, both modes
                combos = [(t, 9, a) for t in THRESHOLDS for a in (False, True)]
            for thr, n_labels, agnostic in combos:
                boxes, labels = _random_inputs(K, 3, n_labels, seed=1000 + 17 * k)
                count = [min(c, K) for c in counts]
                cases.append(_case(f"random-K{K}-count{'-'.join(map(str, count))}-thr{thr}-labels{n_labels}"
                                   f"{'-agnostic' if agnostic else ''}", boxes, labels, thr, agnostic, count=count))
                if K >= 63:                                 # some rows go, some stay
                    c = cases[-1]
                    full = [b for b in range(3) if count[b] == K][0]
                    assert 0 < int(c["want"][4][full]) < K, (c["name"], c["want"][4])
                k += 1
    return cases


# ---- garbage_tail ---------------------------------------------------------------------------------------------------------------
def garbage_tail(case):
    """The same case with everything at or beyond count made hostile: NaN boxes, boxes that would swallow every live one,
    labels of live rows, high scores.  Nothing there may be read: the answer is the case's."""
    c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case.items() if k != "want"}
    B, K = c["scores"].shape
    for b in range(B):
        n = min(max(int(c["count"][b]), 0), K)
        for r in range(n, K):
            c["boxes"][b, r] = (np.nan, 0, np.nan, 1) if (r - n) % 2 else (-1e6, -1e6, 1e6, 1e6)
            c["labels"][b, r] = c["labels"][b, r % n] if n else 0
            c["scores"][b, r] = 9.0
            c["query"][b, r] = 4242
    c["name"] = case["name"] + "-garbage-tail"
    c["want"] = case["want"]
    return c


def clamped_counts():
    """count above K and below 0: n = min(max(count, 0), K)."""
    boxes, labels = _random_inputs(65, 3, 3, seed=77)
    inside = _case("counts-inside", boxes, labels, 0.5, count=[65, 0, 65])
    c = _case("counts-clamped", boxes, labels, 0.5, count=[70, -3, 2 ** 31 - 1])
    for got, want in zip(c["want"], inside["want"]):
        assert got.tobytes() == want.tobytes()
    assert int(c["want"][4][1]) == 0
    return [c]


def all_cases():
    base = strict() + chain() + far() + identical() + disjoint() + degenerate() + random()
    tails = [garbage_tail(c) for c in base if any(int(n) < c["scores"].shape[1] for n in c["count"])]
    # a hand-made case with a tail as well: the chain with its live rows cut off right behind it
    cut = chain()[1]
    cut = _case("chain-at-62-count-65", cut["boxes"], cut["labels"], 0.4, count=[65], kept=[[r for r in range(65) if r != 63]])
    return base + tails + [cut, garbage_tail(cut)] + clamped_counts()


def f64_disagreements(case):
    """Conditioning of a case: the pairs the restatement evaluates on which a float64 `inter / uni > thr` (the usual
    division form, on the same f32 inputs and the f32 threshold) decides differently.  -> (disagreeing, evaluated)"""
    pairs = []
    restate(case["scores"], case["labels"], case["boxes"], case["query"], case["count"], case["thr"], case["agnostic"], pairs)
    thr = float(F(case["thr"]))
    bad = total = 0
    for b, i, j, hit in pairs:
        bx = case["boxes"][b].astype(np.float64)
        with np.errstate(all="ignore"):
            area = np.maximum(bx[:, 2] - bx[:, 0], 0) * np.maximum(bx[:, 3] - bx[:, 1], 0)
            iw = np.maximum(np.minimum(bx[i, 2], bx[j, 2]) - np.maximum(bx[i, 0], bx[j, 0]), 0)
            ih = np.maximum(np.minimum(bx[i, 3], bx[j, 3]) - np.maximum(bx[i, 1], bx[j, 1]), 0)
            inter = iw * ih
            iou = inter / ((area[i] + area[j]) - inter)
        bad += int(((iou > thr) != hit).sum())
        total += hit.size
    return bad, total
