"""Streaming AP (fod_ap_hist_accum / fod_ap_hist_finalize, include/fod_ext.h): a numpy restatement of the definition with
explicit loops -- over the slots for the histograms, over the bins for everything else -- and the cases the CPU and the GPU
tests share.  Nothing here touches future_od.native.ops: the restatement is the header's text, written a second time.

A case is a dict: name, T, C1, batches (a list of (confs f32 [T,C1,P], is_positive u8 [T,C1,P], size_categories u8
[C1,4,P], num_annos i64 [C1,4]), accumulated one after the other into one state) and want = the restatement's
(hist_tp, hist_seen, anno_total, ap, ap101, pr, pr_score, totals).  Cases whose name starts with "unique" draw the keys
of every class without replacement: no two candidates of a row share a bin, and the AP must be the sorted one."""
import functools

import numpy as np

NB = 0x3F81                                # bins
TOP = NB - 1                               # 0x3F80: 1.0 and everything above
POINTS = 101
STATE = ("hist_tp", "hist_seen", "anno_total")
OUTS = ("ap", "ap101", "pr", "pr_score", "totals")
CHUNK, WAVE = 256, 64                      # the finalise walk: 256 bins per round, one scan per 64

# |aggregate_mean_average_precision (float32) - float64 evaluation of the same formula|, greatest over the rows of the
# case, as measured on the CPU (test_ap_hist_cpu.py re-measures it): three times this is what `ap` may differ from the
# float32 function on that case.
F32_DISTANCE = {
    "unique-T1-C2-P65": 6.40e-8,
    "unique-T10-C10-P257": 9.98e-8,
    "unique-T16-C2-P1000": 9.49e-8,
    "unique-T10-C2-P1+63+257": 7.21e-8,
}


def key_of(s):
    """The bin of one f32 score."""
    s = np.float32(s)
    if not s > 0:                          # NaN, zero, negative
        return 0
    return min(int(s.view(np.uint32)) >> 16, TOP)


def edge_of(k):
    return np.uint32(k << 16).view(np.float32)


def score_in(k, low=0):
    """An f32 score of bin k >= 1 (`low`: its 16 truncated bits)."""
    return np.uint32((k << 16) | low).view(np.float32)


def restate_accum(batches, T, C1):
    hist_tp = np.zeros((T, C1, 4, NB), np.int32)
    hist_seen = np.zeros((C1, 4, NB), np.int32)
    anno_total = np.zeros((C1, 4), np.int64)
    for confs, is_pos, sizes, num_annos in batches:
        for c in range(C1):
            for p in range(confs.shape[2]):
                flags = [int(sizes[c, s, p]) for s in range(4)]
                if not any(flags):
                    continue
                k = key_of(confs[0, c, p])
                for s in range(4):
                    if flags[s]:
                        hist_seen[c, s, k] += 1
                        for t in range(T):
                            if is_pos[t, c, p]:
                                hist_tp[t, c, s, k] += 1
        for c in range(C1):
            for s in range(4):
                anno_total[c, s] += num_annos[c, s]
    return hist_tp, hist_seen, anno_total


def restate_finalize(hist_tp, hist_seen, anno_total):
    """Python integers and Python floats (f64), bin by bin.  Empty bins are skipped: they change no sum and, not being
    non-empty, answer no recall point."""
    T, C1 = hist_tp.shape[:2]
    ap = np.full((T, C1, 4), np.nan)
    ap101 = np.full((T, C1, 4), np.nan)
    pr = np.full((T, C1, 4, POINTS), np.nan)
    score = np.full((T, C1, 4, POINTS), np.nan, np.float32)
    totals = np.zeros((T, C1, 4, 2), np.int64)
    for c in range(C1):
        for s in range(4):
            A = int(anno_total[c, s])
            bins = [int(b) for b in np.flatnonzero(hist_seen[c, s])]            # ascending
            se = {b: int(hist_seen[c, s, b]) for b in bins}
            SE, run = {}, 0
            for b in reversed(bins):
                run += se[b]
                SE[b] = run
            for t in range(T):
                totals[t, c, s] = (int(hist_tp[t, c, s].sum(dtype=np.int64)), run)
                if A <= 0:
                    continue
                tp = {b: int(hist_tp[t, c, s, b]) for b in bins}
                TP, up = {}, 0
                for b in reversed(bins):
                    up += tp[b]
                    TP[b] = up
                acc = 0.0
                for b in bins:
                    if tp[b]:
                        acc += float(tp[b]) * (float(TP[b]) / (float(SE[b]) + 1e-5))
                ap[t, c, s] = acc / float(A)
                env, best = {}, -1.0
                for b in bins:
                    best = max(best, float(TP[b]) / float(SE[b]))
                    env[b] = best
                j, total = len(bins) - 1, 0.0                                   # TP falls with the bin: j only moves down
                for i in range(POINTS):
                    while j >= 0 and TP[bins[j]] * 100 < i * A:
                        j -= 1
                    pr[t, c, s, i] = env[bins[j]] if j >= 0 else 0.0
                    score[t, c, s, i] = edge_of(bins[j]) if j >= 0 else 0.0
                    total += pr[t, c, s, i]
                ap101[t, c, s] = total / 101.0
    return ap, ap101, pr, score, totals


def nonempty_bins(hist_tp, hist_seen):
    """n of the bound (n + 3) * 2^-53 per row: [C1,4]."""
    return (hist_seen > 0).sum(axis=2)


def shared_bins(batches, C1):
    """[C1,4] bool: two candidates of the row fall into one bin (all batches together)."""
    _, seen, _ = restate_accum([(b[0][:1], b[1][:1], b[2], b[3]) for b in batches], 1, C1)
    return (seen > 1).any(axis=2)


U = 2.0 ** -53


def assert_exact(got, want, what):
    g = got
    assert g.dtype == want.dtype and g.shape == want.shape, (what, g.dtype, g.shape, want.dtype, want.shape)
    assert np.array_equal(np.isnan(g), np.isnan(want)) if g.dtype.kind == "f" else True, (what, "NaN positions")
    keep = ~np.isnan(want) if g.dtype.kind == "f" else np.ones(want.shape, bool)
    assert g[keep].tobytes() == want[keep].tobytes(), (what, np.argwhere((g != want) & keep)[:8])


def assert_results(state, outs, case, what):
    """The whole comparison of one run (numpy arrays) with the restatement: integers, pr, pr_score and the NaN positions
    byte for byte; ap and ap101 within (n + 3) * 2^-53, n the non-empty bins of the row (101 for ap101) -- non-negative
    terms, a result in [0, 1]."""
    want = dict(zip(STATE + OUTS, case["want"]))
    for name, g in zip(STATE, state):
        assert_exact(g, want[name], (what, case["name"], name))
    ap, ap101, pr, score, totals = outs
    assert_exact(totals, want["totals"], (what, case["name"], "totals"))
    assert_exact(pr, want["pr"], (what, case["name"], "pr"))
    assert_exact(score, want["pr_score"], (what, case["name"], "pr_score"))
    n = nonempty_bins(want["hist_tp"], want["hist_seen"])[None]                  # [1,C1,4]
    for name, g, bound in (("ap", ap, (n + 3) * U), ("ap101", ap101, np.full(n.shape, (101 + 3) * U))):
        w = want[name]
        assert g.dtype == np.float64 and np.array_equal(np.isnan(g), np.isnan(w)), (what, case["name"], name)
        err = np.where(np.isnan(w), 0.0, np.abs(g - w))
        assert (err <= bound).all(), (what, case["name"], name, err.max(), np.argwhere(err > bound)[:8])


# ---- building blocks ------------------------------------------------------------------------------------------------------
def _empty(T, C1, P):
    return (np.zeros((T, C1, P), np.float32), np.zeros((T, C1, P), np.uint8), np.zeros((C1, 4, P), np.uint8),
            np.zeros((C1, 4), np.int64))


def _annos(rng, batch, slack=4):
    """num_annos: at least the true positives of every row at the loosest threshold, plus a few that were missed."""
    confs, is_pos, sizes, num_annos = batch
    tp = (is_pos[0][:, None, :] & sizes).sum(axis=2)
    num_annos[:] = tp + rng.integers(0, slack + 1, size=tp.shape)
    num_annos[:, 0] = np.maximum(num_annos[:, 0], num_annos[:, 1:].sum(axis=1))
    return batch


def random_batch(rng, T, C1, P, unique=False, used=None):
    """Slots as the producers leave them: a filled slot has flag 0 and at most one of flags 1..3, is positive at threshold
    t only if it is at t - 1, and padding is all zeros.  `unique`: the keys of a class are drawn without replacement from
    1..TOP (`used`: per class, the keys of earlier batches)."""
    batch = _empty(T, C1, P)
    confs, is_pos, sizes, _ = batch
    for c in range(C1):
        filled = rng.random(P) < 0.8
        if unique:
            free = np.setdiff1d(np.arange(1, NB), np.fromiter(used[c], int, len(used[c])) if used else [])
            keys = rng.choice(free, size=P, replace=False)
            if used is not None:
                used[c].update(int(k) for k in keys)
            score = np.array([score_in(int(k), int(rng.integers(0, 1 << 16))) for k in keys], np.float32)
            score[keys == TOP] = 1.0
        else:
            score = (rng.random(P) ** 3).astype(np.float32)                 # many low scores, as a sigmoid's
        size = rng.integers(0, 4, P)                                       # 0: a row of non-finite corners, flags (1,0,0,0)
        quality = rng.random(P)
        for p in np.flatnonzero(filled):
            confs[:, c, p] = score[p]
            sizes[c, 0, p] = 1
            if size[p]:
                sizes[c, size[p], p] = 1
            is_pos[:, c, p] = quality[p] > 0.3 + 0.04 * np.arange(T)
    return _annos(rng, batch)


def _case(name, T, C1, batches):
    return dict(name=name, T=T, C1=C1, batches=batches)


def hand_case():
    """Small enough for paper.  Class 0, all sizes: 0.75 (positive), 0.5 (negative), 0.25 (positive), 4 annotations.
    From the top: (TP, SE) = (1, 1), (1, 2), (2, 3); precisions 1, 1/2, 2/3; envelope from below 2/3, 2/3, 1.
    Recall i / 100 needs TP * 100 >= 4 i: i <= 25 is answered by bin 0.75 (1.0), i <= 50 by bin 0.25 (2/3), the rest by
    none.  Size 1 holds the first two with 1 annotation, size 2 the third with 3, size 3 nothing and no annotation.
    Class 1 (generic): one negative at 0.5."""
    confs, is_pos, sizes, num_annos = _empty(1, 2, 4)
    confs[0, 0, :3] = (0.75, 0.5, 0.25)
    confs[0, 1, 0] = 0.5
    is_pos[0, 0, 0] = is_pos[0, 0, 2] = 1
    sizes[0, 0, :3] = 1
    sizes[0, 1, :2] = 1
    sizes[0, 2, 2] = 1
    sizes[1, 0, 0] = 1
    num_annos[:] = ((4, 1, 3, 0), (4, 2, 2, 0))
    return _case("hand", 1, 2, [(confs, is_pos, sizes, num_annos)])


HAND_AP = np.array([[[0.4166636111379627, 0.9999900000999990, 0.3333300000333330, np.nan], [0.0, 0.0, 0.0, np.nan]]])
HAND_AP101 = np.array([[[0.4224422442244224, 1.0, 0.33663366336633666, np.nan], [0.0, 0.0, 0.0, np.nan]]])
HAND_PR_CLASS0_ALL = np.array([1.0] * 26 + [2 / 3] * 25 + [0.0] * 50)
HAND_SCORE_CLASS0_ALL = np.array([0.75] * 26 + [0.25] * 25 + [0.0] * 50, np.float32)
HAND_TOTALS = np.array([[[[2, 3], [1, 2], [1, 1], [0, 0]], [[0, 1], [0, 0], [0, 0], [0, 0]]]], np.int64)

BOUNDARY_KEYS = sorted({0, 1, TOP - 1, TOP} | {k + d for k in range(WAVE, NB, WAVE) for d in (-1, 0)})
ODD_SCORES = (np.nan, -1.0, -0.0, 0.0, -np.inf, np.inf, 1.5, 1.0, 1e-40, 1.1754944e-38, 3.0e38, 0.99999994)


def placed_case():
    """T = 10, C1 = 10, P = 1000, every key put where the kernels have an edge:
    class 0: one candidate in each bin on either side of every 64-bin (wave) and 256-bin (chunk) boundary of the walk,
             plus bins 0, 1, TOP - 1, TOP;  class 1: the same bins, no true positive at all;
    class 2: NaN, negative, zero, infinite, > 1 and subnormal scores;  class 3: every candidate in bin 0 (scores <= 0);
    class 4: 300 candidates in ONE bin, 300 in its neighbour;  class 5: candidates but no annotation (A == 0);
    class 6: no candidate, annotations;  class 7: true positives marked on padding slots (they add nothing);
    classes 8, 9: random."""
    rng = np.random.default_rng(5)
    T, C1, P = 10, 10, 1000
    batch = random_batch(rng, T, C1, P)
    confs, is_pos, sizes, num_annos = batch
    for c in range(8):
        confs[:, c], is_pos[:, c], sizes[c] = 0, 0, 0

    def put(c, p, score, pos, size):
        confs[:, c, p] = score
        sizes[c, 0, p] = 1
        if size:
            sizes[c, size, p] = 1
        is_pos[:pos, c, p] = 1                               # positive at the first `pos` thresholds

    assert len(BOUNDARY_KEYS) <= P
    for c in (0, 1):
        for p, k in enumerate(BOUNDARY_KEYS):
            put(c, p, score_in(k, 0x1234) if k else 0.0, 0 if c else int(rng.integers(0, T + 1)), p % 4)
    for p, s in enumerate(ODD_SCORES):
        put(2, p, s, T if p % 2 else 0, 1 + p % 3)
    for p in range(40):
        put(3, p, -float(p), T if p % 3 == 0 else 0, 1 + p % 3)
    for p in range(600):
        put(4, p, score_in(0x3F00 + p // 300, p), int(rng.integers(0, T + 1)), 1 + p % 3)
    for p in range(30):
        put(5, p, rng.random(), 0, 1 + p % 3)
    is_pos[:, 7, 500:] = 1
    put(7, 3, 0.5, T, 2)
    _annos(rng, batch)
    num_annos[5], num_annos[6], num_annos[0, 3] = 0, (7, 2, 2, 3), 0
    num_annos[1] = (9, 3, 3, 3)
    return _case("placed-T10-C10-P1000", T, C1, [batch])


def _random_case(T, C1, sizes, seed, unique=False):
    rng = np.random.default_rng(seed)
    used = [set() for _ in range(C1)] if unique else None
    name = f"{'unique' if unique else 'random'}-T{T}-C{C1}-P{'+'.join(map(str, sizes))}"
    return _case(name, T, C1, [random_batch(rng, T, C1, P, unique, used) for P in sizes])


def _one_slot_case():
    batch = _empty(16, 2, 1)
    batch[0][:, 0, 0], batch[1][:9, 0, 0], batch[2][0, (0, 3), 0], batch[3][:] = 0.3, 1, 1, ((1, 0, 0, 1), (0, 0, 0, 0))
    return _case("one-slot-T16-C2-P1", 16, 2, [batch])


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = [hand_case(), _one_slot_case(), placed_case(),
             _random_case(1, 2, (63,), 1), _random_case(10, 2, (64,), 2), _random_case(16, 10, (65,), 3),
             _random_case(1, 10, (257,), 4), _random_case(10, 10, (63, 64, 65), 6), _random_case(16, 2, (1000,), 7),
             _random_case(1, 2, (65,), 8, unique=True), _random_case(10, 10, (257,), 9, unique=True),
             _random_case(16, 2, (1000,), 10, unique=True), _random_case(10, 2, (1, 63, 257), 11, unique=True)]
    for case in cases:                                      # computed once, shared by every test, never written to
        state = restate_accum(case["batches"], case["T"], case["C1"])
        case["want"] = state + restate_finalize(*state)
        for a in case["want"] + tuple(x for b in case["batches"] for x in b):
            a.setflags(write=False)
    return tuple(cases)


def concatenated(case):
    """The case's batches as ONE batch: slots side by side, annotations added."""
    bs = case["batches"]
    return tuple(np.concatenate([b[k] for b in bs], axis=2) for k in range(3)) + (sum(b[3] for b in bs),)


def sorted_ap_f64(confs, is_pos, sizes, num_annos):
    """`_get_ap`'s formula (utils/od_map.py) in float64, for every threshold: rank the slots of a class by descending
    score, precision = cumsum(tp) / (cumsum(seen) + 1e-5), AP = sum(precision * tp) / annotations.  -> [T,C1,4]."""
    T, C1, P = confs.shape
    ap = np.full((T, C1, 4), np.nan)
    for t in range(T):
        for c in range(C1):
            order = np.argsort(-confs[t, c].astype(np.float64), kind="stable")
            for s in range(4):
                seen = sizes[c, s, order].astype(np.float64)
                tp = (is_pos[t, c, order] & sizes[c, s, order]).astype(np.float64)
                with np.errstate(invalid="ignore", divide="ignore"):
                    ap[t, c, s] = (np.cumsum(tp) / (np.cumsum(seen) + 1e-5) * tp).sum() / np.float64(num_annos[c, s])
    return ap
