"""Identities across calls on the device: fod_track_update against the numpy restatement of tests/track_cases.py byte for
byte at every call of every case (outputs and state carved out of sentinel-filled buffers, the fields of free slots
hostile), a NULL out_slot, two launches from cloned states, the wrapper's refusals, and the public surface --
DetectionTracker, GraphedTrackedPredict on the small test model of test_predict_gpu.py, render_tracks."""
import numpy as np
import pytest
import torch

import track_cases as TC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = TC.all_cases()
IDS = [c["name"] for c in CASES]
PAD = 3                                    # sentinel elements on either side: 12 bytes, so nothing carved is 16-byte aligned
SENTINELS = {torch.float32: 7.5, torch.int32: -77}


def _carved(array=None, shape=None, dtype=None):
    """A tensor in the middle of a larger sentinel-filled buffer, holding `array` (or sentinels) -> (buffer, tensor)."""
    if array is not None:
        shape, dtype = array.shape, torch.from_numpy(array).dtype
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), SENTINELS[dtype], dtype=dtype, device=DEV)
    t = buf[PAD:PAD + n].view(tuple(shape))
    if array is not None:
        t.copy_(torch.from_numpy(array))
    return buf, t


def _untouched(buf, t):
    s = SENTINELS[buf.dtype]
    return bool((buf[:PAD] == s).all()) and bool((buf[PAD + t.numel():] == s).all())


def _dev(arrays):
    return tuple(torch.from_numpy(a).to(DEV) for a in arrays)


def _assert_equal(got_state, got_outs, want, what):
    for names, got, wanted in ((TC.STATE, got_state, want[0]), (TC.OUTS, got_outs, want[1])):
        for name, g, w in zip(names, got, wanted):
            g = g.cpu().numpy()
            assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
            assert g.tobytes() == w.tobytes(), (what, name, np.argwhere(g != w)[:8])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kernel_equals_the_restatement_at_every_call(case):
    """Every row of every output is written (they start as sentinels), the fields of free slots stay as they were unless
    a track is born there (the restatement leaves them alone), nothing around any tensor is touched."""
    from future_od.native import ops
    carved = [_carved(a) for a in case["state"]]
    state = tuple(t for _, t in carved)
    B, K = case["calls"][0][0].shape
    for i, (inputs, want) in enumerate(zip(case["calls"], case["want"])):
        inputs = _dev(inputs)
        before = [t.clone() for t in inputs]
        outs = [_carved(shape=(B, K), dtype=torch.int32) for _ in range(3)]
        got = ops.track_update(*inputs, state, **TC.params(case), out=tuple(t for _, t in outs))
        _assert_equal(state, got, want, (case["name"], i))
        assert all(_untouched(buf, t) for buf, t in carved + outs), (case["name"], i)
        assert all(torch.equal(a, b) or a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(inputs, before))


SOME = [c for c in CASES if c["name"] in ("second-best", "max-misses-0-cleared-and-reborn", "non-finite-rows")
        or c["name"].startswith(("random-K65-S64-B3", "random-K129-S65-B3", "random-K1024-S1024"))]


@pytest.mark.parametrize("case", SOME, ids=[c["name"] for c in SOME])
def test_null_out_slot_changes_nothing_else_and_two_launches_give_equal_bits(case):
    from future_od.native import ops
    first, second, bare = _dev(case["state"]), _dev(case["state"]), _dev(case["state"])
    for i, (inputs, want) in enumerate(zip(case["calls"], case["want"])):
        inputs = _dev(inputs)
        a = ops.track_update(*inputs, first, **TC.params(case))
        b = ops.track_update(*inputs, second, **TC.params(case))
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(first + a, second + b))
        track, hits = (torch.full_like(inputs[1], -77) for _ in range(2))
        c = ops.track_update(*inputs, bare, **TC.params(case), out=(track, hits))
        assert c[0] is track and c[1] is hits and c[2] is None
        _assert_equal(bare, c[:2], want, (case["name"], i, "no slot"))


def test_wrapper_refuses_bad_operands_before_any_launch():
    from future_od.native import lib as L
    from future_od.native import ops
    case = next(c for c in CASES if c["name"] == "second-best")
    s, l, b, c = _dev(case["calls"][0])
    st = _dev(case["state"])
    kw = TC.params(case)
    other = lambda k, t: st[:k] + (t,) + st[k + 1:]
    before = [t.clone() for t in st]
    L.PROFILER.start()
    for bad in (lambda: ops.track_update(s, l, b, c, st, **{**kw, "iou_threshold": 1.5}),
                lambda: ops.track_update(s, l, b, c, st, **{**kw, "max_misses": -1}),
                lambda: ops.track_update(s, l, b, c.cpu(), st, **kw),
                lambda: ops.track_update(s, l.long(), b, c, st, **kw),
                lambda: ops.track_update(s, l, b[:, :, :3], c, st, **kw),
                lambda: ops.track_update(s, l, b, c, other(2, st[2].cpu()), **kw),
                lambda: ops.track_update(s, l, b, c, other(1, st[0]), **kw),
                lambda: ops.track_update(s, l, b, c, st, **kw, out=(torch.zeros(1), torch.zeros(1)))):
        with pytest.raises(L.FodError, match="track_update"):
            bad()
    launched = [r[0] for r in L.PROFILER.records]
    L.PROFILER.stop()
    assert "fod_track_update" not in launched
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(st, before))


# ---- the model ----------------------------------------------------------------------------------------------------
TOP_K = 100
KW = dict(top_k=TOP_K, nms=0.5, nms_class_agnostic=True)


@pytest.fixture(scope="module")
def model():
    from test_graph_gpu import _build
    return _build("bf16")[0]


def _data(seed):
    from future_od.datasets.synthetic import make_batch
    return make_batch(2, 3, 96, 128, seed=seed, max_boxes=9, device=DEV)


def _tracker():
    from future_od.utils.tracking import DetectionTracker
    return DetectionTracker(2, slots=256, iou_threshold=0.3, max_misses=1, birth_score=0.0, class_agnostic=True)


def test_graphed_tracked_predict_replays_eager_predict_and_update(model):
    """Four successive batches: the graph's dict and the tracker's state equal eager predict + update at every call.
    After the FIRST call next_id is the number of births of ONE update: the warm-up passes of the capture did not leak
    into the state."""
    from future_od.graph import GraphedPredict, GraphedTrackedPredict
    eager, graphed = _tracker(), _tracker()
    gp = GraphedTrackedPredict(model, graphed, **KW)
    assert isinstance(gp, GraphedPredict)
    matched = 0
    for i, seed in enumerate((11, 12, 13, 14)):
        data = _data(seed)
        det = model.predict(data, **KW)
        want = eager.update(det)
        got = gp(data)
        assert set(got) == set(want) == set(det) | {"track", "track_hits"}
        for k in want:
            assert torch.equal(got[k], want[k]), (i, k)
        for k, t in eager.state_dict().items():
            assert torch.equal(graphed.state_dict()[k].view(torch.int32), t.view(torch.int32)), (i, k)
        if i == 0:
            births = (got["track"] >= 0).sum(dim=1).to(torch.int32)
            assert bool((births > 0).all()) and torch.equal(graphed.state_dict()["next_id"], births)
            assert bool((got["track_hits"][got["track"] >= 0] == 1).all())
        matched += int((got["track_hits"] > 1).sum())
        for b in range(2):                                   # padding rows carry no identity
            assert bool((got["track"][b, int(got["count"][b]):] == -1).all())
    assert gp.replays == 4 and len(gp._graphs) == 1
    assert matched > 0                                       # identities did carry over from call to call


def test_tracker_on_predict_without_nms_and_with_attention(model):
    data = _data(11)
    det = model.predict(data, top_k=TOP_K, attention=True)
    tracker = _tracker()
    out = tracker.update(det)
    assert all(out[k] is det[k] for k in det) and out["track"].shape == det["labels"].shape
    assert tracker.device == det["scores"].device
    cpu = _tracker()
    host = cpu.update({k: v.cpu() for k, v in det.items() if k in ("scores", "labels", "boxes", "count")})
    assert torch.equal(out["track"].cpu(), host["track"]) and torch.equal(out["track_hits"].cpu(), host["track_hits"])
    with pytest.raises(ValueError, match="lives on"):
        tracker.update({k: v.cpu() for k, v in det.items()})


def test_render_tracks_on_device_tensors_equals_its_cpu_bytes():
    from future_od.utils import visualization as V
    B, K = 2, 6
    video = torch.randint(0, 256, (B, 2, 3, 96, 128), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    boxes = torch.tensor([[10 + 18 * k, 30 + 3 * k, 40 + 18 * k, 70 + 3 * k] for k in range(K)], dtype=torch.float32)
    det = {"boxes": boxes[None].repeat(B, 1, 1).contiguous(), "scores": torch.full((B, K), 0.37),
           "labels": torch.zeros(B, K, dtype=torch.int32), "count": torch.full((B,), K, dtype=torch.int32),
           "track": torch.tensor([[0, 126, -1, 3, 130, 7], [5, -1, -1, 1, 2, 250]], dtype=torch.int32),
           "track_hits": torch.tensor([[1, 2, 0, 3, 1, 2], [2, 0, 0, 1, 5, 2]], dtype=torch.int32)}
    on = {k: v.to(DEV) for k, v in det.items()}
    frames = torch.tensor([1, 0])
    for kw in (dict(), dict(min_hits=2), dict(captions=V.Captions(ident="slot", scores=True)),
               dict(min_hits=2, captions=V.Captions(scale=1))):
        want = V.render_tracks(video, det, frame_idx=frames, **kw)
        got = V.render_tracks(video.to(DEV), on, frame_idx=frames, **kw)
        assert got.is_cuda and torch.equal(got.cpu(), want), kw
