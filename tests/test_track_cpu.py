"""Identities across calls, the parts that need no GPU: fod_track_update as the binding reads it from include/fod_ext.h and
its argument checks (they return before any launch), ops.track_update on CPU tensors against the numpy restatement of
tests/track_cases.py byte for byte, the hand example, invariants and the conditioning of the random cases,
DetectionTracker, and render_tracks on CPU tensors."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import track_cases as TC
from future_od.native import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, FL = "pointer", "int", "float"
ENTRY = "fod_track_update"
CASES = TC.all_cases()
IDS = [c["name"] for c in CASES]
RANDOM = [c for c in CASES if c["name"].startswith("random")]


# ---- ABI and binding ---------------------------------------------------------------------------------------------------
def test_entry_is_bound_with_the_headers_signature_and_the_abi_moved():
    from future_od.native import lib as L
    hdr = open(os.path.join(ROOT, "include", "fod.h")).read()
    assert int(re.search(r"#define FOD_ABI_VERSION (\d+)", hdr).group(1)) == L.ABI_VERSION == L.LIB.fod_abi_version() >= 19
    assert abi.EXT_PROTOTYPES[ENTRY] == (I, [P, P, P, P, I, I, P, P, P, P, P, I, FL, FL, I, I, I, P, P, P, P])
    assert ENTRY not in abi.PROTOTYPES and ENTRY not in hdr
    ext = open(os.path.join(ROOT, "include", "fod_ext.h")).read()
    proto = re.search(r"\bint\s+fod_track_update\s*\(([^;]*)\);", ext).group(1)
    assert len(proto.split(",")) == len(L.EXT_SIGNATURES[ENTRY]) == 21
    fn = getattr(L.LIB, ENTRY)
    assert fn.restype is abi.CTYPE[I] and list(fn.argtypes) == [abi.CTYPE[k] for k in abi.EXT_PROTOTYPES[ENTRY][1]]


def _entry(B=1, K=4, S=4, thr=0.5, birth=0.5, max_misses=3, null=(), slot=1):
    """The non-null 'pointers' are the address 1: a launch would fault, so a clean non-zero return is the check itself.
    Operands 0..3 are the detections, 4..8 the state, 9..10 out_track and out_hits."""
    from future_od.native import lib as L
    p = [None if k in null else 1 for k in range(11)]
    rc = getattr(L.LIB, ENTRY)(*p[:4], B, K, *p[4:9], S, thr, birth, max_misses, 0, 1, *p[9:], slot, None)
    return rc, L.last_error()


@pytest.mark.parametrize("kw, texts", [
    (dict(K=0), ("K=0", "1..1024")), (dict(K=1025), ("K=1025", "1..1024")), (dict(K=-1), ("K=-1", "1..1024")),
    (dict(S=0), ("S=0", "1..1024")), (dict(S=1025), ("S=1025", "1..1024")), (dict(S=-1), ("S=-1", "1..1024")),
    (dict(B=0), ("B=0", "at least 1")), (dict(B=-2), ("B=-2", "at least 1")),
    (dict(thr=-0.01), ("iou_threshold", "[0, 1]")), (dict(thr=1.5), ("iou_threshold", "[0, 1]")),
    (dict(thr=float("nan")), ("iou_threshold", "[0, 1]")), (dict(thr=float("inf")), ("iou_threshold", "[0, 1]")),
    (dict(max_misses=-1), ("max_misses=-1",)),
] + [(dict(null=(k,)), ("null operand",)) for k in range(11)])
def test_arguments_are_refused_before_any_launch(kw, texts):
    from future_od.native import lib as L
    rc, err = _entry(**kw)
    assert rc == L.ERR_ARG and err.startswith("track_update:") and all(t in err for t in texts), (kw, rc, err)


def test_every_limit_is_checked_with_a_null_slot_too():
    from future_od.native import lib as L
    rc, err = _entry(S=1025, slot=None)
    assert rc == L.ERR_ARG and "1..1024" in err


# ---- the CPU form against the restatement --------------------------------------------------------------------------------
def _t(arrays):
    return tuple(torch.from_numpy(a.copy()) for a in arrays)


def _assert_equal(got_state, got_outs, want, what):
    for names, got, wanted in ((TC.STATE, got_state, want[0]), (TC.OUTS, got_outs, want[1])):
        for name, g, w in zip(names, got, wanted):
            g = g.numpy()
            assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
            assert g.tobytes() == w.tobytes(), (what, name, np.argwhere(g != w)[:8])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cpu_form_equals_the_restatement_at_every_call(case):
    from future_od.native import ops
    state = _t(case["state"])
    for i, (inputs, want) in enumerate(zip(case["calls"], case["want"])):
        inputs = _t(inputs)
        before = [t.clone() for t in inputs]
        outs = tuple(torch.full((inputs[0].shape), -77, dtype=torch.int32) for _ in range(3))     # every row is written
        got = ops.track_update(*inputs, state, **TC.params(case), out=outs)
        assert all(g is o for g, o in zip(got, outs))
        _assert_equal(state, got, want, (case["name"], i))
        assert all(a.numpy().tobytes() == b.numpy().tobytes() for a, b in zip(inputs, before))


def test_out_slot_none_and_fresh_outputs_change_nothing_else():
    from future_od.native import ops
    case = next(c for c in CASES if c["name"].startswith("random-K65-S64-B3"))
    inputs, want = _t(case["calls"][0]), case["want"][0]
    state = _t(case["state"])
    got = ops.track_update(*inputs, state, **TC.params(case))
    _assert_equal(state, got, want, "fresh")
    state = _t(case["state"])
    track, hits = torch.empty(3, 65, dtype=torch.int32), torch.empty(3, 65, dtype=torch.int32)
    got = ops.track_update(*inputs, state, **TC.params(case), out=(track, hits))
    assert got[0] is track and got[1] is hits and got[2] is None
    _assert_equal(state, got[:2], want, "no slot")


def test_wrapper_refuses_bad_operands():
    from future_od.native import lib as L
    from future_od.native import ops
    case = next(c for c in CASES if c["name"] == "second-best")
    s, l, b, c = _t(case["calls"][0])
    st = _t(case["state"])
    kw = TC.params(case)
    run = lambda *a, **k: (lambda: ops.track_update(*a, **{**kw, **k}))
    other = lambda k, t: st[:k] + (t,) + st[k + 1:]
    for bad in (run(s, l, b, c, st, iou_threshold=1.5), run(s, l, b, c, st, iou_threshold=float("nan")),
                run(s, l, b, c, st, iou_threshold=-0.1), run(s, l, b, c, st, max_misses=-1),
                run(s.double(), l, b, c, st), run(s, l.long(), b, c, st), run(s, l, b[:, :, :3], c, st),
                run(s, l, b, c.long(), st), run(s[0], l, b, c, st), run(s, l, b, c, st[:4]),
                run(s, l, b.transpose(1, 2).contiguous().transpose(1, 2), c, st),
                run(s, l, b, c, other(0, st[0][:, :5])), run(s, l, b, c, other(2, st[2].long())),
                run(s, l, b, c, other(3, st[3][:, :, None])), run(s, l, b, c, other(4, st[4].repeat(2))),
                run(s, l, b, c, other(1, st[0])),                                        # one tensor serving twice
                run(s, l, b, c, st, out=(l, torch.zeros_like(l))), run(s, l, b, c, st, out=(torch.zeros_like(l),)),
                run(s, l, b, c, st, out=(torch.zeros_like(l), torch.zeros_like(s))),
                run(torch.zeros(1, 1025), torch.zeros(1, 1025, dtype=torch.int32), torch.zeros(1, 1025, 4), c, st)):
        with pytest.raises(L.FodError, match="track_update"):
            bad()


# ---- the hand example --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("motion", [True, False])
def test_hand_example_comes_out_exactly(motion):
    """One 40 x 40 box of class 2 at score 0.9; iou_threshold 0.3, max_misses 3; seen at x = 100, at x = 110, missed
    twice, seen at x = 140."""
    from future_od.utils.tracking import DetectionTracker
    tracker = DetectionTracker(1, slots=4, iou_threshold=0.3, max_misses=3, birth_score=0.5, motion=motion, device="cpu")
    seen = []
    for x in (100, 110, None, None, 140):
        det = {"scores": torch.tensor([[0.9]]), "labels": torch.tensor([[2]], dtype=torch.int32),
               "boxes": torch.tensor([[[x or 0, 100.0, (x or 0) + 40, 140.0]]]),
               "count": torch.tensor([0 if x is None else 1], dtype=torch.int32)}
        out = tracker.update(det)
        seen.append((int(out["track"][0, 0]), int(out["track_hits"][0, 0])))
    if motion:
        assert seen == [(0, 1), (0, 2), (-1, 0), (-1, 0), (0, 3)] and int(tracker.state_dict()["next_id"][0]) == 1
        live = tracker.tracks()
        assert live["id"].tolist() == [0] and live["boxes"].tolist() == [[140.0, 100.0, 180.0, 140.0]]
        assert live["vel"].tolist() == [[10.0, 0.0, 10.0, 0.0]] and live["label"].tolist() == [2]
    else:
        # [140, 180] against the last associated [110, 150]: inter 10 x 40, union 70 x 40 -- IoU 1/7, below 0.3
        assert seen == [(0, 1), (0, 2), (-1, 0), (-1, 0), (1, 1)] and int(tracker.state_dict()["next_id"][0]) == 2
        assert sorted(tracker.tracks()["id"].tolist()) == [0, 1]


def test_a_track_missed_max_misses_plus_one_times_is_cleared_and_its_slot_reused():
    case = next(c for c in CASES if c["name"] == "cleared-and-reused")
    metas = [w[0][2][0, 0].tolist() for w in case["want"]]
    assert metas == [[0, 0, 1, 0], [0, 0, 1, 1], [0, 0, 1, 2], [-1, -1, 0, 0], [1, 1, 1, 0]]


# ---- invariants and conditioning of the random cases -----------------------------------------------------------------------
@pytest.mark.parametrize("case", RANDOM, ids=[c["name"] for c in RANDOM])
def test_invariants_and_float64_conditioning(case):
    """Ids are unique among the live slots of a sample, next_id never decreases, every match has inter > 0 -- and, a
    property of THESE inputs (the seeds of track_cases.scene were kept because it holds for them): with the division
    and everything before it in float64 on the same float32 predicted boxes, every claim is made the same way, so no
    outcome of the random cases hangs on a rounding."""
    state = case["state"]
    for inputs in case["calls"]:
        claims = []
        after, outs = TC.restate(*inputs, state, case["thr"], case["birth"], case["max_misses"], case["agnostic"],
                                 case["motion"], claims=claims)
        _, wide = TC.restate(*inputs, state, case["thr"], case["birth"], case["max_misses"], case["agnostic"],
                             case["motion"], wide=True)
        for name, a, w in zip(TC.OUTS, outs, wide):
            assert a.tobytes() == w.tobytes(), (case["name"], name)
        assert all(inter > 0 for _, _, _, inter in claims)
        assert len(claims) == int((outs[1] > 1).sum())                    # a matched row has been seen before
        for b in range(after[2].shape[0]):
            ids = after[2][b, :, 0]
            ids = ids[ids >= 0]
            assert len(set(ids.tolist())) == ids.size and (ids < after[4][b]).all()
            tracked = outs[0][b][outs[0][b] >= 0]
            assert len(set(tracked.tolist())) == tracked.size            # no identity on two rows of one call
        assert (after[4] >= state[4]).all()
        state = after


def test_the_random_cases_reach_every_kind_of_row():
    m, b, u = (sum(x) for x in zip(*(TC.matched_rows(c) for c in RANDOM)))
    assert m > 1000 and b > 1000 and u > 1000


# ---- DetectionTracker ---------------------------------------------------------------------------------------------------
def _det(case, i=0):
    s, l, b, c = _t(case["calls"][i])
    return {"scores": s, "labels": l, "boxes": b, "count": c, "query": torch.arange(s.numel(), dtype=torch.int32).view(s.shape)}


def _tracker(case, **kw):
    from future_od.utils.tracking import DetectionTracker
    B, S = case["state"][0].shape[:2]
    return DetectionTracker(B, slots=S, **TC.params(case), **kw)


SEQ = next(c for c in CASES if c["name"].startswith("random-K64-S65-B3"))


def test_tracker_update_returns_a_new_dict_and_leaves_det_untouched():
    tracker = _tracker(SEQ)                                # no device given: the first update's
    state = _clean(SEQ)
    for i in range(len(SEQ["calls"])):
        det = _det(SEQ, i)
        keys, before = set(det), {k: v.clone() for k, v in det.items()}
        out = tracker.update(det)
        assert out is not det and set(det) == keys and set(out) == keys | {"track", "track_hits"}
        assert all(out[k] is det[k] and torch.equal(det[k], before[k]) for k in keys)
        # an empty tracker is the hostile empty state without its garbage: the same identities
        state, want = TC.restate(*SEQ["calls"][i], state, SEQ["thr"], SEQ["birth"], SEQ["max_misses"], SEQ["agnostic"],
                                 SEQ["motion"])
        assert out["track"].numpy().tobytes() == want[0].tobytes()
        assert out["track_hits"].numpy().tobytes() == want[1].tobytes()
    for name, w in zip(TC.STATE, state):
        assert tracker.state_dict()[name].numpy().tobytes() == w.tobytes(), name


def _clean(case):
    B, S = case["state"][0].shape[:2]
    meta = np.zeros((B, S, 4), np.int32)
    meta[:, :, :2] = -1
    return [np.zeros((B, S, 4), TC.F), np.zeros((B, S, 4), TC.F), meta, np.zeros((B, S), TC.F), np.zeros(B, np.int32)]


def test_tracker_reset_state_dict_snapshot_and_restore():
    tracker = _tracker(SEQ, device="cpu")
    empty = tracker.state_dict()
    assert tracker.tracks()["id"].numel() == 0
    tracker.update(_det(SEQ, 0))
    tracker.update(_det(SEQ, 1))
    two = tracker.state_dict()
    assert (two["next_id"] > 0).all() and not torch.equal(two["meta"], empty["meta"])
    live = tracker.tracks()
    assert live["id"].numel() == int((two["meta"][:, :, 0] >= 0).sum()) and (live["hits"] >= 1).all()
    assert torch.equal(live["boxes"], two["boxes"][live["sample"], live["slot"]])
    # reset(sample) clears that sample only
    tracker.reset(1)
    now = tracker.state_dict()
    for k in TC.STATE:
        assert torch.equal(now[k][1], empty[k][1]) and torch.equal(now[k][0], two[k][0]) and torch.equal(now[k][2], two[k][2])
    # load_state_dict copies INTO the tensors the tracker owns; the round trip continues as if nothing had happened
    owned = tracker._tensors()
    tracker.load_state_dict(two)
    assert all(a is b for a, b in zip(owned, tracker._tensors()))
    snap = tracker.snapshot()
    third = tracker.update(_det(SEQ, 2))
    after = tracker.state_dict()
    tracker.restore(snap)
    assert all(torch.equal(tracker.state_dict()[k], two[k]) for k in TC.STATE)
    again = tracker.update(_det(SEQ, 2))
    assert torch.equal(again["track"], third["track"]) and torch.equal(again["track_hits"], third["track_hits"])
    assert all(torch.equal(tracker.state_dict()[k], after[k]) for k in TC.STATE)
    other = _tracker(SEQ, device="cpu")
    other.load_state_dict(after)
    assert all(torch.equal(other.state_dict()[k], after[k]) for k in TC.STATE)
    tracker.reset()
    assert all(torch.equal(tracker.state_dict()[k], empty[k]) for k in TC.STATE)


def test_tracker_refusals():
    from future_od.utils.tracking import DetectionTracker
    for kw in (dict(batch=0), dict(batch=1, slots=0), dict(batch=1, slots=1025), dict(batch=1, iou_threshold=1.5),
               dict(batch=1, iou_threshold=float("nan")), dict(batch=1, max_misses=-1)):
        with pytest.raises(ValueError, match="DetectionTracker"):
            DetectionTracker(**kw)
    tracker = _tracker(SEQ, device="cpu")
    det = _det(SEQ)
    with pytest.raises(ValueError, match="batch of 3"):
        tracker.update({k: v[:2].contiguous() for k, v in det.items()})
    with pytest.raises(ValueError, match="lives on cpu"):
        tracker.to_device("meta")
    with pytest.raises(ValueError, match="sample 3"):
        tracker.reset(3)
    with pytest.raises(ValueError, match="state\\['meta'\\]"):
        tracker.load_state_dict({**tracker.state_dict(), "meta": torch.zeros(3, 4, 4, dtype=torch.int32)})
    with pytest.raises(ValueError, match="no state yet"):
        _tracker(SEQ).tracks()


def test_no_parameter_was_added_to_predict_or_its_graphed_form():
    from future_od.graph import GraphedPredict, GraphedTrackedPredict
    from future_od.models.st_detr import SpatioTemporalDETR
    assert "tracker" not in inspect.signature(SpatioTemporalDETR.predict).parameters
    assert "tracker" not in inspect.signature(GraphedPredict.__init__).parameters
    own = list(inspect.signature(GraphedTrackedPredict.__init__).parameters)
    assert own[:3] == ["self", "model", "tracker"] and own[3:] == list(inspect.signature(GraphedPredict.__init__).parameters)[2:]
    assert issubclass(GraphedTrackedPredict, GraphedPredict) and "__init__" in vars(GraphedTrackedPredict)


# ---- render_tracks ----------------------------------------------------------------------------------------------------------
def test_render_tracks_on_cpu_tensors_is_render_with_the_stated_labels_and_idents():
    from future_od.utils import visualization as V
    B, K = 2, 6
    video = torch.randint(0, 256, (B, 2, 3, 96, 128), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    boxes = torch.tensor([[10 + 18 * k, 30 + 3 * k, 40 + 18 * k, 70 + 3 * k] for k in range(K)], dtype=torch.float32)
    det = {"boxes": boxes[None].repeat(B, 1, 1).contiguous(), "scores": torch.full((B, K), 0.37),
           "labels": torch.zeros(B, K, dtype=torch.int32), "count": torch.full((B,), K, dtype=torch.int32),
           "track": torch.tensor([[0, 126, -1, 3, 130, 7], [5, -1, -1, 1, 2, 250]], dtype=torch.int32),
           "track_hits": torch.tensor([[1, 2, 0, 3, 1, 2], [2, 0, 0, 1, 5, 2]], dtype=torch.int32)}
    P = V.COLOURS.shape[0]
    for min_hits in (1, 2):
        labels = torch.where((det["track"] >= 0) & (det["track_hits"] >= min_hits), det["track"] % P,
                             torch.full_like(det["track"], -1))
        assert torch.equal(V.track_colour_index(det, min_hits), labels)
        assert labels[0].tolist() == ([0, 1, -1, 3, 5, 7] if min_hits == 1 else [-1, 1, -1, 3, -1, 7])
        frames = torch.tensor([1, 0])
        plain = V.render_tracks(video, det, min_hits=min_hits, frame_idx=frames)
        assert torch.equal(plain, V.render(video, det["boxes"], labels, frame_idx=frames))
        for cap in (V.Captions(ident="slot"), V.Captions(scores=True, scale=1)):
            got = V.render_tracks(video, det, min_hits=min_hits, frame_idx=frames, captions=cap)
            scores = det["scores"] if cap.scores is True else False
            want = V.render(video, det["boxes"], labels, frame_idx=frames,
                            captions=V.Captions(ident=det["track"], scores=scores, scale=cap.scale))
            assert torch.equal(got, want) and not torch.equal(got, plain)
    # the colour follows the identity: the same track in another row, another class, another call -- the same colour
    assert not torch.equal(V.render_tracks(video, det), V.render(video, det["boxes"], det["labels"]))
    with pytest.raises(ValueError, match="names"):
        V.render_tracks(video, det, captions=V.Captions(names=["car"]))
