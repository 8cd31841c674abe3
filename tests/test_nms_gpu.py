"""Duplicate suppression on the device: fod_detect_nms against the numpy restatement of tests/nms_cases.py byte for byte
(fresh outputs inside a sentinel-filled buffer, a second launch, outputs aliasing the inputs, a NULL source), and the
public surface -- predict(nms=...), GraphedPredict(nms=...), the launch list, the attention rows, render_detections -- on
the small test model of test_predict_gpu.py."""
import numpy as np
import pytest
import torch

import nms_cases as NC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = NC.all_cases()
IDS = [c["name"] for c in CASES]
OLD_KEYS = ("scores", "labels", "boxes", "query", "count")
PAD = 3                                    # sentinel elements on either side of an output: 12 bytes, so no output is 16-byte aligned
SENTINELS = {torch.float32: 7.5, torch.int32: 77}


def _inputs(case):
    return tuple(torch.from_numpy(case[k]).to(DEV) for k in NC.NAMES[:5])


def _carved(shape, dtype):
    """A tensor of `shape` in the middle of a larger sentinel-filled buffer -> (buffer, tensor)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), SENTINELS[dtype], dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + n].view(shape)


def _outputs(case):
    B, K = case["scores"].shape
    shapes = (((B, K), torch.float32), ((B, K), torch.int32), ((B, K, 4), torch.float32), ((B, K), torch.int32),
              ((B,), torch.int32), ((B, K), torch.int32))
    pairs = [_carved(s, d) for s, d in shapes]
    return [p[0] for p in pairs], tuple(p[1] for p in pairs)


def _assert_equal(got, case, what):
    for name, g, w in zip(NC.NAMES, got, case["want"]):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        assert g.tobytes() == w.tobytes(), (what, case["name"], name, g, w)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kernel_equals_the_restatement(case):
    from future_od.native import ops
    inputs = _inputs(case)
    before = [t.clone() for t in inputs]
    bufs, outs = _outputs(case)
    got = ops.detect_nms(*inputs, case["thr"], case["agnostic"], out=outs)
    assert all(g is o for g, o in zip(got, outs))
    _assert_equal(got, case, "fresh outputs")
    for buf, o in zip(bufs, outs):                          # the bytes around every output are untouched
        s = SENTINELS[buf.dtype]
        assert bool((buf[:PAD] == s).all()) and bool((buf[PAD + o.numel():] == s).all()), case["name"]
    for t, b in zip(inputs, before):                        # ... and so are the inputs
        assert t.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    # a second launch into other memory: equal bits
    second = ops.detect_nms(*inputs, case["thr"], case["agnostic"])
    for a, b in zip(second, got):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    # the outputs are the inputs
    source = torch.full(inputs[1].shape, 77, dtype=torch.int32, device=DEV)
    again = ops.detect_nms(*inputs, case["thr"], case["agnostic"], out=inputs + (source,))
    assert all(a is o for a, o in zip(again, inputs + (source,)))
    _assert_equal(again, case, "in place")
    # ... and once more on what that left: a suppressed result is a fixed point (its survivors do not suppress each other)
    fixed = ops.detect_nms(*inputs, case["thr"], case["agnostic"])
    for name, a, w in zip(NC.NAMES[:5], fixed, case["want"]):
        assert a.cpu().numpy().tobytes() == w.tobytes(), (case["name"], name)


@pytest.mark.parametrize("name", ["chain-at-63", "degenerate", "random-K300-count300-150-3-thr0.5-labels9", "far-0-1023"])
def test_null_source_is_accepted_and_changes_nothing_else(name):
    from future_od.native import lib as L
    from future_od.native import ops
    case = next(c for c in CASES if c["name"] == name)
    inputs = _inputs(case)
    B, K = case["scores"].shape
    bufs, outs = _outputs(case)
    L.call("fod_detect_nms", *(ops.ptr(t) for t in inputs), B, K, float(case["thr"]), int(case["agnostic"]),
           *(ops.ptr(t) for t in outs[:5]), None, ops.stream())
    torch.cuda.synchronize()
    _assert_equal(outs[:5], case, "null source")
    assert bool((bufs[5] == SENTINELS[torch.int32]).all())
    for buf, o in zip(bufs[:5], outs[:5]):
        s = SENTINELS[buf.dtype]
        assert bool((buf[:PAD] == s).all()) and bool((buf[PAD + o.numel():] == s).all())


def test_wrapper_refuses_bad_device_operands():
    from future_od.native import lib as L
    from future_od.native import ops
    s, l, b, q, c = _inputs(CASES[0])
    for bad in (lambda: ops.detect_nms(s, l, b, q, c, 1.5), lambda: ops.detect_nms(s, l, b, q, c.cpu()),
                lambda: ops.detect_nms(s, l.long(), b, q, c), lambda: ops.detect_nms(s, l, b[:, :, :3], q, c),
                lambda: ops.detect_nms(s, l, b, q, c, out=(s, l, b, q, c, torch.zeros(s.shape, dtype=torch.int32)))):
        with pytest.raises(L.FodError, match="detect_nms"):
            bad()


# ---- the model ----------------------------------------------------------------------------------------------------
TOP_K = 300                                 # >= 2 * num_queries (128): the same query comes back under several classes


@pytest.fixture(scope="module")
def model():
    from test_graph_gpu import _build
    return _build("bf16")[0]


def _data(seed=11):
    from future_od.datasets.synthetic import make_batch
    return make_batch(2, 3, 96, 128, seed=seed, max_boxes=9, device=DEV)


def _same(a, b, keys):
    return set(a) == set(b) == set(keys) and all(torch.equal(a[k], b[k]) for k in keys)


@pytest.mark.parametrize("agnostic", [False, True])
def test_predict_with_nms_is_detect_nms_on_predict(model, agnostic):
    from future_od.native import ops
    data = _data()
    plain = model.predict(data, top_k=TOP_K)
    assert set(plain) == set(OLD_KEYS)
    want = ops.detect_nms(*(plain[k] for k in OLD_KEYS), 0.5, agnostic)
    det = model.predict(data, top_k=TOP_K, nms=0.5, nms_class_agnostic=agnostic)
    assert set(det) == set(OLD_KEYS) | {"source"} and det["source"].dtype == torch.int32
    for k, w in zip(OLD_KEYS + ("source",), want):
        assert det[k].cpu().numpy().tobytes() == w.cpu().numpy().tobytes(), k
    again = model.predict(data, top_k=TOP_K)                 # the option leaves nothing behind
    assert _same(again, plain, OLD_KEYS)
    if agnostic:
        assert bool((det["count"] < plain["count"]).all())   # (see the next test: there were duplicates)


def test_class_agnostic_nms_returns_no_query_twice(model):
    data = _data()
    plain = model.predict(data, top_k=TOP_K)
    det = model.predict(data, top_k=TOP_K, nms=0.5, nms_class_agnostic=True)

    def repeated(d, b):
        n = int(d["count"][b])
        bx = d["boxes"][b, :n]
        positive = ((bx[:, 2] > bx[:, 0]) & (bx[:, 3] > bx[:, 1])).cpu()
        q = d["query"][b, :n].cpu()[positive]
        return int(q.numel() - q.unique().numel())
    for b in range(2):
        assert repeated(plain, b) > 0                        # duplicates existed before suppression
        assert repeated(det, b) == 0
        assert 0 < int(det["count"][b]) < int(plain["count"][b])


def test_launch_lists(model):
    from future_od.native import lib as L
    data = _data()
    lists = {}
    for name, kw in (("plain", {}), ("nms", dict(nms=0.5)), ("attention", dict(attention=True)),
                     ("both", dict(nms=0.5, attention=True)), ("after", {})):
        L.PROFILER.start()
        out = model.predict(data, top_k=TOP_K, **kw)
        lists[name] = ([r[0] for r in L.PROFILER.records], set(out))
    L.PROFILER.stop()
    plain, keys = lists["plain"]
    assert keys == set(OLD_KEYS) and lists["after"] == (plain, keys)
    assert "fod_detect_nms" not in plain and plain.count("fod_detect_select") == 1 and plain[-1] == "fod_detect_select"
    at = plain.index("fod_detect_select") + 1
    assert lists["nms"] == (plain[:at] + ["fod_detect_nms"] + plain[at:], keys | {"source"})
    assert lists["attention"] == (plain + ["fod_attn_maps"], keys | {"attention", "attention_frames"})
    assert lists["both"] == (plain + ["fod_detect_nms", "fod_attn_maps"], keys | {"source", "attention", "attention_frames"})


def test_attention_rows_follow_the_survivors(model):
    data = _data()
    plain = model.predict(data, top_k=TOP_K, attention=True)
    det = model.predict(data, top_k=TOP_K, attention=True, nms=0.5, nms_class_agnostic=True)
    assert det["attention"].shape == plain["attention"].shape
    assert torch.equal(det["attention_frames"], plain["attention_frames"])
    for b in range(2):
        m = int(det["count"][b])
        assert 0 < m < int(plain["count"][b])
        src = det["source"][b, :m].long()
        assert torch.equal(det["attention"][b, :m], plain["attention"][b, src])
        assert float(det["attention"][b, :m].sum()) > 0
        assert not bool(det["attention"][b, m:].any())       # padding rows are zero
        assert bool((det["source"][b, m:] == -1).all())


def test_graphed_predict_with_nms_replays_eager_predict(model):
    from future_od.graph import GraphedPredict
    keys = OLD_KEYS + ("source",)
    gp = GraphedPredict(model, top_k=TOP_K, nms=0.5, nms_class_agnostic=True)
    counts = []
    for d in (_data(11), _data(12)):
        want = model.predict(d, top_k=TOP_K, nms=0.5, nms_class_agnostic=True)
        got = gp(d)
        assert _same(got, want, keys)
        counts.append(got["count"].tolist())
        assert all(0 < c < TOP_K for c in counts[-1])
    assert len(gp._graphs) == 1 and gp.replays == 2
    assert set(GraphedPredict(model, top_k=TOP_K)(_data(11))) == set(OLD_KEYS)      # off by default
    aware = GraphedPredict(model, top_k=TOP_K, nms=0.5)
    assert _same(aware(_data(12)), model.predict(_data(12), top_k=TOP_K, nms=0.5), keys)


def test_render_detections_draws_exactly_the_survivors(model):
    from future_od.utils import visualization as V
    data = _data()
    plain = model.predict(data, top_k=TOP_K)
    det = model.predict(data, top_k=TOP_K, nms=0.5, nms_class_agnostic=True)
    got = V.render_detections(data["video"], det, min_score=0.0)
    # the survivors, taken from the UNSUPPRESSED result through `source`, as plain boxes and labels
    m = det["count"].tolist()
    boxes = torch.zeros(2, max(m), 4, device=DEV)
    labels = torch.full((2, max(m)), -1, dtype=torch.int32, device=DEV)
    for b in range(2):
        src = det["source"][b, :m[b]].long()
        boxes[b, :m[b]], labels[b, :m[b]] = plain["boxes"][b, src], plain["labels"][b, src]
    want = V.render(data["video"], boxes, labels)
    assert got.dtype == torch.uint8 and torch.equal(got, want)
    everything = V.render_detections(data["video"], plain, min_score=0.0)
    assert everything.shape == got.shape
