"""Identities across calls (fod_track_update, include/fod_ext.h): a numpy float32 restatement of the definition and the
cases the CPU form and the kernel are held against.  It is written from the header and shares no helper with the
package.  Every operation of the restatement is explicitly np.float32 and rounded once, so equality of every state
tensor and every output byte is the right comparison: no tolerance appears anywhere.

A case is a dict: name, K, S, the parameters (thr, birth, max_misses, agnostic, motion), state = the five state arrays
BEFORE the first call (boxes f32 [B,S,4], vel f32 [B,S,4], meta i32 [B,S,4], scores f32 [B,S], next_id i32 [B]), calls =
a list of (scores f32 [B,K], labels i32 [B,K], boxes f32 [B,K,4], count i32 [B]) and want = per call (the five state
arrays after it, (track, hits, slot)).  The state is threaded through the calls.  The fields of free slots hold hostile
values (a box that swallows every row, NaN velocities, the rows' own labels): nothing may read them, and nothing may
write them unless a track is born there -- the restatement leaves them alone, so equal bytes check exactly that.
Cases whose answer is known by hand assert it here, on the restatement, when the case is built."""
import numpy as np

F = np.float32
STATE = ("boxes", "vel", "meta", "scores", "next_id")
OUTS = ("track", "hits", "slot")


def _iou(row, pred, wide):
    """inter and IoU of one row box with every predicted box [S,4], operation for operation as the header has them; `wide`:
    the same expression in float64 on the same float32 boxes (the conditioning check of test_track_cpu.py)."""
    T = np.float64 if wide else F
    row, pred, zero = row.astype(T), pred.astype(T), T(0)
    with np.errstate(all="ignore"):
        area_r = np.maximum(row[2] - row[0], zero) * np.maximum(row[3] - row[1], zero)
        area_p = np.maximum(pred[:, 2] - pred[:, 0], zero) * np.maximum(pred[:, 3] - pred[:, 1], zero)
        inter = (np.maximum(np.minimum(row[2], pred[:, 2]) - np.maximum(row[0], pred[:, 0]), zero) *
                 np.maximum(np.minimum(row[3], pred[:, 3]) - np.maximum(row[1], pred[:, 1]), zero))
        uni = (area_r + area_p) - inter
        ok = uni > 0
        iou = np.where(ok, inter / np.where(ok, uni, T(1)), zero)
    assert inter.dtype == iou.dtype == T
    return inter, iou


def restate(scores, labels, boxes, count, state, thr, birth, max_misses, agnostic, motion, wide=False, claims=None):
    """One call.  `state`: the five arrays; they are NOT modified.  -> (the five arrays after the call, (track, hits,
    slot)).  `claims` (a list) receives (b, row, slot, inter) of every match."""
    tb, tv, tm, ts, nid = (a.copy() for a in state)
    B, K = scores.shape
    S = tb.shape[1]
    assert scores.dtype == boxes.dtype == tb.dtype == tv.dtype == ts.dtype == F
    assert labels.dtype == count.dtype == tm.dtype == nid.dtype == np.int32
    track, hits, slot = np.full((B, K), -1, np.int32), np.zeros((B, K), np.int32), np.full((B, K), -1, np.int32)
    thr, birth = F(thr), F(birth)
    for b in range(B):
        n = min(max(int(count[b]), 0), K)                   # rows at or beyond n are never read
        live = [s for s in range(S) if tm[b, s, 0] >= 0]
        # 1. prediction
        pred, gaps, open_ = np.zeros((S, 4), F), np.ones(S, F), np.zeros(S, bool)
        for s in live:
            gaps[s] = F(int(tm[b, s, 3]) + 1)
            with np.errstate(all="ignore"):
                p = tb[b, s] + tv[b, s] * gaps[s] if motion else tb[b, s].copy()
            assert p.dtype == F
            if np.isfinite(p).all():
                pred[s], open_[s] = p, True
        # 2. claims, in row order
        by_row, by_slot = {}, {}
        for j in range(n):
            if not np.isfinite(boxes[b, j]).all():
                continue
            seen = [s for s in live if open_[s] and s not in by_slot and (agnostic or tm[b, s, 1] == labels[b, j])]
            if not seen:
                continue
            inter, iou = _iou(boxes[b, j], pred[seen], wide)
            k = int(np.flatnonzero(iou == iou.max())[0])     # the greatest IoU, ties to the lowest slot (seen ascends)
            if inter[k] > 0 and iou[k] >= thr:
                by_row[j], by_slot[seen[k]] = seen[k], j
                if claims is not None:
                    claims.append((b, j, seen[k], float(inter[k])))
        # 3. matched slots, 4. the others age
        for s in live:
            if s in by_slot:
                j = by_slot[s]
                with np.errstate(all="ignore"):
                    tv[b, s] = (boxes[b, j] - tb[b, s]) / gaps[s] if motion else F(0)
                tb[b, s], ts[b, s] = boxes[b, j], scores[b, j]
                tm[b, s, 1], tm[b, s, 2], tm[b, s, 3] = labels[b, j], tm[b, s, 2] + 1, 0
                track[b, j], hits[b, j], slot[b, j] = tm[b, s, 0], tm[b, s, 2], s
            else:
                tm[b, s, 3] += 1
                if tm[b, s, 3] > max_misses:
                    tm[b, s], tb[b, s], tv[b, s], ts[b, s] = (-1, -1, 0, 0), F(0), F(0), F(0)
        # 5. births
        free = [s for s in range(S) if tm[b, s, 0] < 0]
        cand = [j for j in range(n) if j not in by_row and np.isfinite(boxes[b, j]).all() and scores[b, j] >= birth]
        for r, (j, s) in enumerate(zip(cand, free)):
            tb[b, s], tv[b, s], ts[b, s] = boxes[b, j], F(0), scores[b, j]
            tm[b, s] = (nid[b] + r, labels[b, j], 1, 0)
            track[b, j], hits[b, j], slot[b, j] = nid[b] + r, 1, s
        nid[b] += min(len(cand), len(free))
    return (tb, tv, tm, ts, nid), (track, hits, slot)


# ---- building cases -----------------------------------------------------------------------------------------------------------
def hostile_state(B, S, labels=(0, 1, 2)):
    """An empty state whose free slots hold what must never be read."""
    tb = np.tile(np.array([-1e6, -1e6, 1e6, 1e6], F), (B, S, 1))
    tv = np.full((B, S, 4), np.nan, F)
    tm = np.zeros((B, S, 4), np.int32)
    tm[:, :, 0] = -1 - (np.arange(S, dtype=np.int32) % 3)[None]          # any negative id is free
    tm[:, :, 1] = np.asarray(labels, np.int32)[np.arange(S) % len(labels)][None]
    tm[:, :, 2], tm[:, :, 3] = 12345, 777
    ts = np.full((B, S), 9.0, F)
    return [tb, tv, tm, ts, np.zeros(B, np.int32)]


def put_track(state, b, s, ident, label, box, vel=(0, 0, 0, 0), hits=1, misses=0, score=0.5):
    state[0][b, s], state[1][b, s], state[2][b, s], state[3][b, s] = box, vel, (ident, label, hits, misses), score
    state[4][b] = max(int(state[4][b]), ident + 1)


def call(rows, K=None, count=None):
    """rows: per sample a list of (box, label, score) -> (scores, labels, boxes, count) with hostile padding."""
    if rows and not isinstance(rows[0], list):
        rows = [rows]
    B = len(rows)
    K = max(1, max(len(r) for r in rows)) if K is None else K
    scores, labels = np.full((B, K), 9.0, F), np.zeros((B, K), np.int32)
    boxes = np.tile(np.array([-1e6, -1e6, 1e6, 1e6], F), (B, K, 1))
    for b, rs in enumerate(rows):
        for j, (box, label, score) in enumerate(rs):
            boxes[b, j], labels[b, j], scores[b, j] = box, label, score
    cnt = np.array([len(r) for r in rows] if count is None else count, np.int32)
    return scores, labels, np.ascontiguousarray(boxes), cnt


def make_case(name, state, calls, thr=0.3, birth=0.5, max_misses=3, agnostic=False, motion=True, tracks=None, slots=None,
              next_id=None):
    """`tracks` / `slots`: per call, per sample, what the rows must come out as (hand cases); `next_id`: after the last."""
    K, S = calls[0][0].shape[1], state[0].shape[1]
    c = dict(name=name, K=K, S=S, thr=thr, birth=birth, max_misses=max_misses, agnostic=bool(agnostic), motion=bool(motion),
             state=[a.copy() for a in state], calls=calls, want=[])
    cur = state
    for i, (scores, labels, boxes, count) in enumerate(calls):
        cur, outs = restate(scores, labels, boxes, count, cur, thr, birth, max_misses, agnostic, motion)
        c["want"].append((cur, outs))
        for what, hand, got in (("track", tracks, outs[0]), ("slot", slots, outs[2])):
            if hand is not None and hand[i] is not None:
                for b, row in enumerate(hand[i] if isinstance(hand[i][0], list) else [hand[i]]):
                    assert got[b, :len(row)].tolist() == list(row), (name, what, i, b, got[b, :len(row)].tolist())
    if next_id is not None:
        assert cur[4].tolist() == list(next_id), (name, cur[4].tolist())
    return c


def params(case):
    return dict(iou_threshold=case["thr"], birth_score=case["birth"], max_misses=case["max_misses"],
                class_agnostic=case["agnostic"], motion=case["motion"])


# ---- hand cases ---------------------------------------------------------------------------------------------------------------
A, Bx = [0, 0, 10, 10], [4, 0, 14, 10]
FAR = [[500 + 20 * i, 500, 510 + 20 * i, 510] for i in range(8)]


def hand_example(motion):
    """The worked example: one 40 x 40 box of class 2 at score 0.9, seen, seen 10 further right, missed twice, seen
    30 further right.  With the motion model the prediction [140, 100, 180, 140] is where it is found: one identity.
    Without it the last sighting has IoU 1/7 with the last associated box: a new identity."""
    seen = lambda x: call([([x, 100, x + 40, 140], 2, 0.9)])
    calls = [seen(100), seen(110), call([[]]), call([[]]), seen(140)]
    last = 0 if motion else 1
    c = make_case(f"hand-example-motion{int(motion)}", hostile_state(1, 4), calls, thr=0.3, max_misses=3, motion=motion,
                  tracks=[[0], [0], [-1], [-1], [last]], next_id=[last + 1])
    assert [int(w[1][1][0, 0]) for w in c["want"]] == [1, 2, 0, 0, 3 if motion else 1]
    return c


def hand():
    cases = [hand_example(True), hand_example(False)]
    # no live slot: births in row order into ascending free slots; a score below birth_score stays untracked
    cases.append(make_case("no-live-slot", hostile_state(1, 4), [call([(FAR[0], 0, 0.9), (FAR[1], 1, 0.4), (FAR[2], 2, 0.5)])],
                           tracks=[[0, -1, 1]], slots=[[0, -1, 1]], next_id=[2]))
    # every slot live, nothing matches: births overflow, nothing is born
    st = hostile_state(1, 2)
    put_track(st, 0, 0, 7, 0, A)
    put_track(st, 0, 1, 8, 0, Bx)
    cases.append(make_case("full-births-overflow", st, [call([(FAR[0], 0, 0.9), (FAR[1], 0, 0.9), (FAR[2], 0, 0.9)])],
                           tracks=[[-1, -1, -1]], next_id=[9]))
    # ... with max_misses = 0 both are cleared in this call and their slots are born in again at once
    cases.append(make_case("max-misses-0-cleared-and-reborn", st,
                           [call([(FAR[0], 0, 0.9), (FAR[1], 0, 0.9), (FAR[2], 0, 0.9)])], max_misses=0,
                           tracks=[[9, 10, -1]], slots=[[0, 1, -1]], next_id=[11]))
    # ... and one of them is matched: only the other is cleared, and the first newborn gets it
    cases.append(make_case("max-misses-0-one-matched", st, [call([(FAR[0], 0, 0.9), (A, 0, 0.9), (FAR[2], 0, 0.9)])],
                           max_misses=0, tracks=[[9, 7, -1]], slots=[[1, 0, -1]], next_id=[10]))
    # two identical tracks: the tie goes to the lowest slot, the second identical row takes the other
    st = hostile_state(1, 70)
    put_track(st, 0, 66, 5, 1, A)
    put_track(st, 0, 3, 6, 1, A)
    put_track(st, 0, 65, 4, 1, A)
    cases.append(make_case("identical-tracks-tie", st, [call([(A, 1, 0.9), (A, 1, 0.8), (A, 1, 0.7), (A, 1, 0.6)])],
                           tracks=[[6, 4, 5, 7]], slots=[[3, 65, 66, 0]]))
    # the best slot of row 1 (A: 9/11) was claimed by row 0: it takes its second best (B: 7/13)
    st = hostile_state(1, 130)
    put_track(st, 0, 129, 0, 0, A)
    put_track(st, 0, 64, 1, 0, Bx)
    cases.append(make_case("second-best", st, [call([(A, 0, 0.9), ([1, 0, 11, 10], 0, 0.8)])],
                           tracks=[[0, 1]], slots=[[129, 64]]))
    # ... and with a threshold above 7/13 it takes nothing and is born
    cases.append(make_case("second-best-below-threshold", st, [call([(A, 0, 0.9), ([1, 0, 11, 10], 0, 0.8)])], thr=0.6,
                           tracks=[[0, 2]], slots=[[129, 0]]))
    # a best IoU below the threshold (2/18) claims nothing: the later row takes that slot
    st = hostile_state(1, 3)
    put_track(st, 0, 1, 0, 0, A)
    cases.append(make_case("below-threshold-leaves-slot", st, [call([([8, 0, 18, 10], 0, 0.9), (A, 0, 0.8)])],
                           tracks=[[1, 0]], slots=[[0, 1]]))
    # IoU exactly equal to the threshold on small integers: it matches (>=)
    for thr, row in ((0.5, [0, 0, 2, 1]), (0.25, [0, 0, 1, 1])):
        st = hostile_state(1, 1)
        put_track(st, 0, 0, 3, 0, [0, 0, 2, 2])
        cases.append(make_case(f"iou-equals-threshold-{thr}", st, [call([(row, 0, 0.9)])], thr=thr, tracks=[[3]]))
    # threshold 0: disjoint and merely touching boxes have inter == 0 and do not match; any overlap does
    st = hostile_state(1, 2)
    put_track(st, 0, 0, 3, 0, A)
    cases.append(make_case("threshold-0", st, [call([([10, 0, 20, 10], 0, 0.1), ([30, 0, 40, 10], 0, 0.1),
                                                     ([9.5, 9.5, 20, 20], 0, 0.1)])], thr=0.0, tracks=[[-1, -1, 3]]))
    # threshold 1: only the identical box
    st = hostile_state(1, 2)
    put_track(st, 0, 0, 3, 0, A)
    put_track(st, 0, 1, 4, 0, [100, 0, 110, 10])
    cases.append(make_case("threshold-1", st, [call([([0, 0, 10, 9.5], 0, 0.1), (A, 0, 0.1), ([100, 0, 110, 10], 0, 0.1)])],
                           thr=1.0, tracks=[[-1, 3, 4]]))
    # zero-area and inverted boxes match nothing, as rows and as tracks; they are born like any row
    st = hostile_state(1, 5)
    put_track(st, 0, 0, 0, 0, [5, 5, 5, 9])
    put_track(st, 0, 1, 1, 0, [10, 10, 6, 6])
    put_track(st, 0, 2, 2, 0, [6, 6, 10, 10])
    cases.append(make_case("zero-area-and-inverted", st, [call([([5, 5, 5, 9], 0, 0.9), ([10, 10, 6, 6], 0, 0.9),
                                                                ([6, 6, 10, 10], 0, 0.9), ([5, 5, 5, 9], 0, 0.9)])],
                           thr=0.0, tracks=[[3, 4, 2, -1]], slots=[[3, 4, 2, -1]]))
    # non-finite rows claim nothing and are never born; a NaN score matches (scores are never compared) but is never born
    nan, inf = float("nan"), float("inf")
    st = hostile_state(1, 8)
    put_track(st, 0, 0, 0, 0, [6, 6, 10, 10])
    put_track(st, 0, 1, 1, 0, [200, 200, 210, 210])
    cases.append(make_case("non-finite-rows", st, [call([([6, 6, nan, 10], 0, 0.9), ([-inf, 6, 10, 10], 0, 0.9),
                                                         ([6, 6, 10, 10], 0, nan), ([300, 300, 310, 310], 0, nan),
                                                         ([200, 200, 210, inf], 0, 0.9), ([200, 200, 210, 210], 0, inf)])],
                           tracks=[[-1, -1, 0, -1, -1, 1]], next_id=[2]))
    # a slot whose predicted box overflows cannot be claimed and ages; without the motion model it is claimed
    for motion in (True, False):
        st = hostile_state(1, 2)
        put_track(st, 0, 0, 0, 0, [1e37, 0, 1.1e37, 10], vel=[3e38, 0, 3e38, 0], misses=1)
        cases.append(make_case(f"prediction-overflows-motion{int(motion)}", st, [call([([1e37, 0, 1.1e37, 10], 0, 0.9)])],
                               motion=motion, tracks=[[1 if motion else 0]]))
    # class-aware: another class does not match and is born; class-agnostic: it matches and the track takes the row's class
    for agnostic in (False, True):
        st = hostile_state(1, 2)
        put_track(st, 0, 1, 0, 2, A)
        c = make_case(f"other-class-agnostic{int(agnostic)}", st, [call([(A, 3, 0.9)])], agnostic=agnostic,
                      tracks=[[0 if agnostic else 1]], slots=[[1 if agnostic else 0]])
        assert c["want"][0][0][2][0, 1].tolist() == ([0, 3, 2, 0] if agnostic else [0, 2, 1, 1])
        cases.append(c)
    # gaps of 1, 2 and 3: the velocity after a sighting is the displacement divided by the calls since the last one
    for misses in (0, 1, 2):
        st = hostile_state(1, 1)
        put_track(st, 0, 0, 0, 0, [0, 0, 30, 30], misses=misses)
        c = make_case(f"gap-{misses + 1}", st, [call([([7, 1, 37, 31], 0, 0.9)])], tracks=[[0]])
        gap = F(misses + 1)
        assert c["want"][0][0][1][0, 0].tolist() == [F(7) / gap, F(1) / gap, F(7) / gap, F(1) / gap]
        cases.append(c)
    # a track missed max_misses + 1 times is cleared, and its slot is used again
    st = hostile_state(1, 1)
    c = make_case("cleared-and-reused", st, [call([(A, 0, 0.9)])] + [call([[]])] * 3 + [call([(FAR[0], 1, 0.9)])],
                  max_misses=2, tracks=[[0], [-1], [-1], [-1], [1]], slots=[[0], [-1], [-1], [-1], [0]], next_id=[2])
    assert c["want"][2][0][2][0, 0].tolist() == [0, 0, 1, 2] and c["want"][3][0][2][0, 0].tolist() == [-1, -1, 0, 0]
    cases.append(c)
    return cases


def counts():
    """count 0, negative and above K; everything at or beyond n is hostile and never read."""
    rows = [(A, 0, 0.9), (FAR[0], 0, 0.9)]
    st = hostile_state(3, 3)
    for b in range(3):
        put_track(st, b, 2, 4, 0, A)
    return [make_case("counts-0-negative-above", st, [call([rows, rows, rows], K=5, count=[0, -3, 2 ** 31 - 1])],
                      tracks=[[[-1] * 5, [-1] * 5, [4, 5, 6, -1, -1]]], next_id=[5, 5, 7])]


# ---- random sequences ---------------------------------------------------------------------------------------------------------
SIZES = ((1, 1), (1, 63), (63, 1), (64, 64), (65, 64), (64, 65), (63, 129), (129, 65), (300, 256))      # (K, S)
BIG = ((1024, 129), (129, 1024), (1024, 1024))


def scene(K, S, B, calls, seed, n_labels=3, fill=0.6):
    """Objects that drift with a velocity of their own; every call sees most of them, jittered, among clutter, rows in
    descending score order.  Objects sit in clusters, so that rows compete for the same tracks."""
    rng = np.random.RandomState(seed)
    n_obj = max(1, int(min(K, S) * fill))
    n_clusters = max(1, n_obj // 3)
    centres = rng.uniform([100, 100], [1500, 800], size=(B, n_clusters, 2))
    which = rng.randint(0, n_clusters, size=(B, n_obj))
    pos = centres[np.arange(B)[:, None], which] + rng.uniform(-25, 25, size=(B, n_obj, 2))
    size = rng.uniform(30, 120, size=(B, n_obj, 2))
    vel = rng.uniform(-9, 9, size=(B, n_obj, 2))
    cls = rng.randint(0, n_labels, size=(B, n_obj))
    out = []
    for t in range(calls):
        scores, labels = np.zeros((B, K), F), np.full((B, K), -1, np.int32)
        boxes = np.zeros((B, K, 4), F)
        count = np.zeros(B, np.int32)
        for b in range(B):
            c = pos[b] + vel[b] * t + rng.uniform(-3, 3, size=(n_obj, 2))
            s = size[b] * rng.uniform(0.95, 1.05, size=(n_obj, 2))
            bx = np.concatenate([c - s / 2, c + s / 2], axis=1)
            lb = cls[b].copy()
            n_clutter = rng.randint(0, max(1, K - n_obj) + 1)
            cc = rng.uniform([0, 0], [1600, 900], size=(n_clutter, 2))
            cs = rng.uniform(20, 90, size=(n_clutter, 2))
            bx = np.concatenate([bx[rng.uniform(size=n_obj) < 0.85], np.concatenate([cc - cs / 2, cc + cs / 2], axis=1)])[:K]
            lb = np.concatenate([lb, rng.randint(0, n_labels, size=n_clutter)])[:len(bx)]
            sc = np.sort(rng.uniform(0.05, 0.99, size=len(bx)))[::-1]
            order = rng.permutation(len(bx))
            n = len(bx)
            boxes[b, :n], labels[b, :n], scores[b, :n], count[b] = bx[order], lb[order], sc, n
        out.append((scores, labels, boxes, count))
    return out


def random():
    cases = []
    for k, (K, S) in enumerate(SIZES):
        for B in (1, 3):
            thr, agnostic, motion = (0.3, 0.5, 0.7)[k % 3], bool((k + B) % 2), bool((k // 2 + B) % 2 == 0)
            cases.append(make_case(f"random-K{K}-S{S}-B{B}-thr{thr}-agnostic{int(agnostic)}-motion{int(motion)}",
                                   hostile_state(B, S), scene(K, S, B, 5, seed=100 + 7 * k + B), thr=thr, birth=0.4,
                                   max_misses=(3, 1, 0)[k % 3], agnostic=agnostic, motion=motion))
    for k, (K, S) in enumerate(BIG):                       # the limits: two calls, the second on a populated state
        cases.append(make_case(f"random-K{K}-S{S}-B1", hostile_state(1, S), scene(K, S, 1, 2, seed=900 + k), thr=0.3,
                               birth=0.3, max_misses=2, agnostic=bool(k % 2), motion=True))
    return cases


def all_cases():
    return hand() + counts() + random()


def matched_rows(case):
    """How many rows the restatement matched, born, and left alone, over all calls: (matched, born, untracked)."""
    m = bo = u = 0
    for (_, (track, hits, _)), (_, _, _, count) in zip(case["want"], case["calls"]):
        m += int(((track >= 0) & (hits > 1)).sum())
        bo += int(((track >= 0) & (hits == 1)).sum())
        u += int((track < 0).sum())
    return m, bo, u
