"""AP bookkeeping over detection rows on the device: fod_detect_od_map against the numpy restatement of
tests/detect_eval_cases.py byte for byte (outputs carved from sentinel-filled buffers, a second launch, a captured launch
replayed on changed rows), against the existing fod_od_map where nothing is cut, and the public surface --
prepare_od_map_detections, DetectionEvaluator, Trainer.evaluate_detections -- on the small models of the existing tests."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import detect_eval_cases as DC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = DC.all_cases()
IDS = [c["name"] for c in CASES]
GROUP1 = [c for c in CASES if c["name"].startswith("all-pairs")]
PAD = 3                                    # sentinel elements on either side of an output: no f32 / u8 output is 16-byte aligned
SENTINELS = {torch.float32: 7.5, torch.uint8: 77, torch.int64: 77}
OLD_KEYS = ("scores", "labels", "boxes", "query", "count")


def _inputs(case):
    return tuple(torch.from_numpy(case[k]).to(DEV) for k in DC.ROWS + DC.ANNOS)


def _shapes(case):
    B, C1, P, T = case["scores"].shape[0], case["C"] + 1, case["P"], case["T"]
    return (((T, C1, B * P), torch.float32), ((T, C1, B * P), torch.uint8), ((C1, 4, B * P), torch.uint8),
            ((C1, 4), torch.int64))


def _carved(shape, dtype):
    """A tensor of `shape` in the middle of a larger sentinel-filled buffer -> (buffer, tensor)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), SENTINELS[dtype], dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + n].view(shape)


def _assert_equal(got, case, what):
    for name, g, w in zip(DC.OUTS, got, case["want"]):
        g = g.cpu().numpy()
        g = g.view(np.uint8) if g.dtype == np.bool_ else g
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, case["name"], name, np.argwhere(g != w)[:8])


def _same_bits(a, b):
    """torch.equal that lets NaN equal NaN (an AP of a class without annotations)."""
    return a.dtype == b.dtype and a.shape == b.shape and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def _run(case, inputs, **kw):
    from future_od.native import ops
    return ops.detect_od_map(*inputs, case["imsize"], case["C"], case["per_class"], T=case["T"], **kw)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kernel_equals_the_restatement(case):
    inputs = _inputs(case)
    before = [t.clone() for t in inputs]
    pairs = [_carved(s, d) for s, d in _shapes(case)]
    bufs, outs = [p[0] for p in pairs], tuple(p[1] for p in pairs)
    assert any(o.data_ptr() % 16 for o in outs[:3])
    got = _run(case, inputs, out=outs)
    assert all(g is o for g, o in zip(got, outs))
    _assert_equal(got, case, "carved outputs")
    for buf, o in zip(bufs, outs):                          # the bytes around every output are untouched
        s = SENTINELS[buf.dtype]
        assert bool((buf[:PAD] == s).all()) and bool((buf[PAD + o.numel():] == s).all()), case["name"]
    for t, b in zip(inputs, before):                        # ... and so are the inputs
        assert t.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    # a second launch into other (uninitialised) memory: equal bits
    second = _run(case, inputs)
    assert second[1].dtype == second[2].dtype == torch.bool
    _assert_equal(second, case, "second launch")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_captured_launch_replays_on_changed_rows(case):
    """The launch as a graph node: captured on one set of rows, replayed on another (the first sample's rows reversed, its
    count lowered) -- the replay gives the restatement's bytes for what the buffers hold then."""
    static = [t.clone() for t in _inputs(case)]
    outs = tuple(torch.full(s, 9, dtype=d, device=DEV) for s, d in _shapes(case))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _run(case, static, out=outs)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _run(case, static, out=outs)
    for o in outs:
        o.fill_(9)
    graph.replay()
    _assert_equal(outs, case, "first replay")
    other = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    n = min(max(int(case["count"][0]), 0), case["scores"].shape[1])
    for k in DC.ROWS[:4]:
        other[k][0, :n] = case[k][0, :n][::-1]
    other["count"][0] = max(n - 1, 0)
    other["want"] = DC.restate(*(other[k] for k in DC.ROWS + DC.ANNOS), case["imsize"], case["C"], case["P"], case["T"])
    assert any(a.tobytes() != b.tobytes() for a, b in zip(other["want"], case["want"]))
    for s, k in zip(static, DC.ROWS + DC.ANNOS):
        s.copy_(torch.from_numpy(other[k]))
    graph.replay()
    _assert_equal(outs, other, "replay on changed rows")


@pytest.mark.parametrize("case", GROUP1, ids=[c["name"] for c in GROUP1])
def test_all_pairs_selected_equals_the_existing_kernel(case):
    """detect_select with every pair, then detect_od_map == post_proc, then od_map, on the same logits and boxes."""
    from future_od.native import ops
    H, W = case["imsize"]
    logits, cxcywh = torch.from_numpy(case["logits"]).to(DEV), torch.from_numpy(case["cxcywh"]).to(DEV)
    annos = _inputs(case)[5:]
    B, M, C = logits.shape
    rows = ops.detect_select(logits, cxcywh, H, W, top_k=M * C, score_threshold=0.0)
    assert rows[4].tolist() == [M * C] * B
    got = ops.detect_od_map(*rows, *annos, (H, W), C, per_class=min(50, M))
    scores, boxes_px = ops.post_proc(logits, cxcywh, H, W)
    want = ops.od_map(scores, boxes_px, *annos, (H, W))
    for name, g, w in zip(DC.OUTS, got, want):
        assert g.dtype == w.dtype and torch.equal(g, w), (case["name"], name)
    assert bool(got[1][0].any()) and not bool(got[1][0].all())


def test_wrapper_refuses_bad_device_operands():
    from future_od.native import lib as L
    from future_od.native import ops
    case = CASES[0]
    s, l, b, q, c, ab, ac, aa = _inputs(case)
    im, C = case["imsize"], case["C"]
    for bad in (lambda: ops.detect_od_map(s, l, b, q, c.cpu(), ab, ac, aa, im, C),
                lambda: ops.detect_od_map(s, l, b, q, c, ab.cpu(), ac, aa, im, C),
                lambda: ops.detect_od_map(s, l.long(), b, q, c, ab, ac, aa, im, C),
                lambda: ops.detect_od_map(s, l, b, q, c, ab, ac, aa, im, C, out=tuple(torch.zeros(1) for _ in range(4)))):
        with pytest.raises(L.FodError, match="detect_od_map"):
            bad()


# ---- the model ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from test_graph_gpu import _build
    return _build("bf16")[0]


def _data(seed=11):
    from future_od.datasets.synthetic import make_batch
    return make_batch(2, 3, 96, 128, seed=seed, max_boxes=9, device=DEV)


M, C = 128, 8                              # the test model's queries and classes: M * C = 1024 rows is every pair


def test_every_pair_through_predict_is_the_od_of_forward(model):
    from future_od.utils.od_map import prepare_od_map_detections
    data = _data()
    with torch.no_grad():
        od = model(data=data, distributed=False)[4]
    det = model.predict(data, top_k=M * C)
    got = prepare_od_map_detections(det, data["boxes"], data["classes"], data["active"], (96, 128), C)
    assert len(got) == len(od) == 4
    for name, g, w in zip(DC.OUTS, got, od):
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w), name
    assert bool(got[2][:, 0].all())                         # no padding: every class has M >= 50 rows


def test_graphed_predict_with_the_evaluator_equals_the_eager_form(model):
    from future_od.graph import GraphedPredict
    from future_od.utils.od_map import DetectionEvaluator
    kw = dict(top_k=300, nms=0.5)
    gp = GraphedPredict(model, **kw)
    graphed, eager = DetectionEvaluator(C), DetectionEvaluator(C)
    for seed in (11, 12):
        graphed.update(gp(_data(seed)), _data(seed))
        eager.update(model.predict(_data(seed), **kw), _data(seed))
    assert len(gp._graphs) == 1 and gp.replays == 2 and len(graphed) == len(eager) == 2
    for a, b in zip(graphed.tensors(), eager.tensors()):
        assert torch.equal(a, b)
    assert graphed.tensors()[0].shape == (10, C + 1, 2 * 2 * 50) and graphed.tensors()[3].shape == (C + 1, 4, 2)
    a, b = graphed.aggregate("cpu"), eager.aggregate("cpu")
    assert set(a) == set(b) and _same_bits(a["all"], b["all"]) and _same_bits(a["generic"], b["generic"])
    op = a["operating_point"]
    assert op["detections"].shape == (C + 1,) and int(op["annotations"][-1]) == int(op["annotations"][:-1].sum()) > 0
    assert 0 < int(op["detections"][-1]) <= 2 * 2 * 50 and int(op["true_positives"][-1]) <= int(op["annotations"][-1])


def test_launch_lists_are_what_they_were(model):
    from future_od.graph import GraphedPredict
    from future_od.native import lib as L
    from future_od.utils.od_map import DetectionEvaluator
    data = _data()
    lists = {}
    for name, kw in (("plain", {}), ("nms", dict(nms=0.5)), ("after", {})):
        L.PROFILER.start()
        out = model.predict(data, top_k=300, **kw)
        lists[name] = ([r[0] for r in L.PROFILER.records], set(out))
        if name == "nms":                                    # the evaluation is ONE launch of its own, behind predict's
            DetectionEvaluator(C).update(out, data)
            assert [r[0] for r in L.PROFILER.records] == lists[name][0] + ["fod_detect_od_map"]
    L.PROFILER.start()
    with torch.no_grad():
        model(data=data, distributed=False)
    forward = [r[0] for r in L.PROFILER.records]
    L.PROFILER.stop()
    plain, keys = lists["plain"]
    assert keys == set(OLD_KEYS) and lists["after"] == (plain, keys)
    assert "fod_detect_od_map" not in plain + lists["nms"][0] + forward and forward.count("fod_od_map") == 1
    assert plain[-1] == "fod_detect_select" and lists["nms"] == (plain + ["fod_detect_nms"], keys | {"source"})
    gp = GraphedPredict(model, top_k=300)
    assert set(gp(data)) == set(OLD_KEYS)


# ---- the trainer ------------------------------------------------------------------------------------------------------
class _Loader(list):
    batch_size = 2


def test_trainer_evaluate_detections(tmp_path, capsys):
    from future_od.datasets.synthetic import make_batch
    from future_od.models.st_detr import SpatioTemporalDETRArgs
    from future_od.trainer import Trainer
    from runs._helper import get_lr_func, setup_optimizer
    from runs._model import build_model
    torch.manual_seed(0)
    args = SimpleNamespace(device=DEV, distributed=False, compute_dtype="bf16", backbone="resnet18")
    detr = SpatioTemporalDETRArgs(num_classes=8, num_queries=32, lr_backbone=1e-4, enc_layers=1, dec_layers=2,
                                  pretrained_backbone=False)
    net = build_model(args, detr)
    sched, opt = setup_optimizer(detr, net, get_lr_func(4))
    batches = [make_batch(2, 3, 96, 128, seed=s, max_boxes=5) for s in (1, 2)]
    tr = Trainer(net, opt, sched, _Loader(batches), {"val": _Loader(batches), "other": _Loader(batches[:1])}, str(tmp_path),
                 str(tmp_path), "t", DEV, print_interval=3, visualization_epochs=[], visualization_iterations=[],
                 category_dict={}, is_master=True, max_norm=detr.max_norm)
    net.to(DEV)
    net.train()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    plain = tr.evaluate_detections(top_k=256)
    assert net.training                                      # the mode it was in
    after = net.state_dict()
    assert set(after) == set(before) and all(torch.equal(before[k], after[k]) for k in before)
    assert set(plain) == {"val", "other"}
    for name, images in (("val", 4), ("other", 2)):
        ap = plain[name]
        assert set(ap) == {"all", "classavg", "threshavg", "classavg threshavg", "generic", "generic threshavg",
                           "operating_point"}
        assert ap["all"].shape == (10, 8, 4) and ap["generic"].shape == (10, 4)
        assert int(ap["operating_point"]["detections"][-1]) == images * 32          # every query once, none cut (P = 50)
    text = capsys.readouterr().out
    assert text.count("AP50 for epoch is:") == 2 and text.count("MAP for large objects is:") == 2
    assert text.count("Precision / recall at IoU 0.5") == 2
    nms = tr.evaluate_detections(top_k=256, nms=0.5, nms_class_agnostic=True)
    a, b = plain["val"]["operating_point"], nms["val"]["operating_point"]
    assert torch.equal(a["annotations"], b["annotations"]) and int(a["annotations"][-1]) > 0
    # every query came back under all 8 classes with one box: class-agnostic suppression leaves at most one of them
    assert int(b["detections"][:-1].sum()) < int(a["detections"][:-1].sum()) and int(b["detections"][-1]) <= int(a["detections"][-1])
    assert all(torch.equal(before[k], v) for k, v in net.state_dict().items())
    # where the evaluation pass would not be captured, eager predict gives the same numbers
    tr._eval_graph_allowed = lambda: False
    eager = tr.evaluate_detections(top_k=256)
    for name in plain:
        assert _same_bits(eager[name]["all"], plain[name]["all"])
        assert torch.equal(eager[name]["operating_point"]["true_positives"], plain[name]["operating_point"]["true_positives"])
