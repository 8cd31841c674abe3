"""Streaming AP on the device: fod_ap_hist_accum / fod_ap_hist_finalize against the numpy restatement of
tests/ap_hist_cases.py (integers, pr, pr_score and NaN positions byte for byte, ap and ap101 within (n + 3) * 2^-53; the
state carved from sentinel-filled buffers, a second run, the two launches as nodes of a captured graph), the tie to the
sorted AP, and the public surface -- StreamingDetectionEvaluator against DetectionEvaluator on rows of `predict`, the
launch lists, the trainer's switch -- on the small models of the existing tests."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import ap_hist_cases as AC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = AC.all_cases()
IDS = [c["name"] for c in CASES]
UNIQUE = [c for c in CASES if c["name"].startswith("unique")]
PAD = 5                                    # sentinel elements on either side of a state tensor
SENTINEL = 77


def _od(batch, flags=torch.uint8):
    confs, is_pos, sizes, num_annos = (torch.from_numpy(a.copy()).to(DEV) for a in batch)
    return confs, is_pos.to(flags), sizes.to(flags), num_annos


def _carved_state(T, C1):
    """A zeroed state in the middle of larger sentinel-filled buffers -> (buffers, state)."""
    bufs, state = [], []
    for shape, dtype in (((T, C1, 4, AC.NB), torch.int32), ((C1, 4, AC.NB), torch.int32), ((C1, 4), torch.int64)):
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=dtype, device=DEV)
        buf[PAD:PAD + n] = 0
        bufs.append(buf)
        state.append(buf[PAD:PAD + n].view(shape))
    return bufs, tuple(state)


def _numpy(tensors):
    return [t.cpu().numpy() for t in tensors]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kernels_equal_the_restatement(case):
    from future_od.native import ops
    bufs, state = _carved_state(case["T"], case["C1"])
    batches = [_od(b) for b in case["batches"]]
    before = [[t.clone() for t in b] for b in batches]
    for b in batches:
        assert ops.ap_hist_accum(b, state) is state
    kept = [t.clone() for t in state]
    outs = ops.ap_hist_finalize(state)
    assert [o.dtype for o in outs] == [torch.float64, torch.float64, torch.float64, torch.float32, torch.int64]
    AC.assert_results(_numpy(state), _numpy(outs), case, "kernels")
    for buf, t in zip(bufs, state):                          # the elements around the state are untouched
        assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[PAD + t.numel():] == SENTINEL).all()), case["name"]
    for b, w in zip(batches, before):                        # ... and so are the inputs, and finalise reads the state only
        assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(b, w))     # (a NaN score stays one)
    assert all(torch.equal(x, y) for x, y in zip(state, kept))
    # a second run -- bool flags, the batches in reverse, then as one concatenated batch: equal bits
    for other in ([_od(b, torch.bool) for b in case["batches"]][::-1], [_od(AC.concatenated(case))]):
        again = ops.ap_hist_state(case["T"], case["C1"], DEV)
        for b in other:
            ops.ap_hist_accum(b, again)
        assert all(torch.equal(x, y) for x, y in zip(again, state))
        for x, y in zip(ops.ap_hist_finalize(again), outs):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


def test_cpu_form_and_kernel_agree_on_the_integers_and_the_curve():
    from future_od.native import ops
    case = next(c for c in CASES if c["name"].startswith("placed"))
    host = ops.ap_hist_state(case["T"], case["C1"], "cpu")
    dev = ops.ap_hist_state(case["T"], case["C1"], DEV)
    for b in case["batches"]:
        ops.ap_hist_accum(tuple(torch.from_numpy(a.copy()) for a in b), host)
        ops.ap_hist_accum(_od(b), dev)
    assert all(torch.equal(a, b.cpu()) for a, b in zip(host, dev))
    h, d = ops.ap_hist_finalize(host), ops.ap_hist_finalize(dev)
    for k in (2, 3, 4):                                      # pr, pr_score, totals
        assert h[k].numpy().tobytes() == d[k].cpu().numpy().tobytes()


def test_captured_launches_replay():
    """Both launches as graph nodes: three accumulations and the finalisation captured once; every replay on a zeroed
    state gives the restatement's bytes, on the batches the static buffers hold at that time."""
    from future_od.native import ops
    case = next(c for c in CASES if len(c["batches"]) == 3)
    static = [_od(b) for b in case["batches"]]
    state = ops.ap_hist_state(case["T"], case["C1"], DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for b in static:
            ops.ap_hist_accum(b, state)
        ops.ap_hist_finalize(state)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for b in static:
            ops.ap_hist_accum(b, state)
        outs = ops.ap_hist_finalize(state)
    for t in state:
        t.zero_()
    graph.replay()
    AC.assert_results(_numpy(state), _numpy(outs), case, "first replay")
    # other rows in the same buffers: the first batch's scores moved on by one slot
    first = case["batches"][0]
    other = dict(case, batches=[(np.roll(first[0], 1, axis=2),) + tuple(first[1:])] + list(case["batches"][1:]))
    want_state = AC.restate_accum(other["batches"], case["T"], case["C1"])
    other["want"] = want_state + AC.restate_finalize(*want_state)
    assert want_state[1].tobytes() != case["want"][1].tobytes()
    for s, a in zip(static[0], other["batches"][0]):
        s.copy_(torch.from_numpy(a.copy()))
    for t in state:
        t.zero_()
    graph.replay()
    AC.assert_results(_numpy(state), _numpy(outs), other, "replay on changed rows")


@pytest.mark.parametrize("case", UNIQUE, ids=[c["name"] for c in UNIQUE])
def test_ap_is_the_sorted_ap_where_no_bin_is_shared(case):
    from future_od.native import ops
    from future_od.utils.od_map import aggregate_mean_average_precision
    state = ops.ap_hist_state(case["T"], case["C1"], DEV)
    for b in case["batches"]:
        ops.ap_hist_accum(_od(b), state)
    ap = ops.ap_hist_finalize(state)[0].cpu().numpy()
    od = AC.concatenated(case)
    exact = AC.sorted_ap_f64(*od)
    n = AC.nonempty_bins(case["want"][0], case["want"][1])[None]
    assert np.array_equal(np.isnan(ap), np.isnan(exact))
    err = np.where(np.isnan(exact), 0.0, np.abs(ap - exact))
    print(f"{case['name']}: |ap - float64 sorted AP| <= {err.max():.3e}")
    assert (err <= (n + 3) * AC.U).all(), (case["name"], err.max())
    t = tuple(torch.from_numpy(a.copy()) for a in od)
    table = aggregate_mean_average_precision(t[0], t[1].bool(), t[2].bool(), t[3][:, :, None], "cpu")
    f32 = torch.cat([table["all"], table["generic"][:, None]], dim=1).numpy().astype(np.float64)
    finite = ~np.isnan(exact) & np.isfinite(f32)
    print(f"{case['name']}: |ap - float32 AP| <= {np.abs(ap - f32)[finite].max():.3e}, limit {3 * AC.F32_DISTANCE[case['name']]:.3e}")
    assert np.abs(ap - f32)[finite].max() <= 3 * AC.F32_DISTANCE[case["name"]]


def test_wrappers_refuse_bad_device_operands():
    from future_od.native import lib as L
    from future_od.native import ops
    confs, is_pos, sizes, num_annos = _od(AC.hand_case()["batches"][0])
    state = ops.ap_hist_state(1, 2, DEV)
    for bad in (lambda: ops.ap_hist_accum((confs.cpu(), is_pos, sizes, num_annos), state),
                lambda: ops.ap_hist_accum((confs, is_pos, sizes, num_annos.cpu()), state),
                lambda: ops.ap_hist_accum((confs, is_pos, sizes, num_annos), ops.ap_hist_state(1, 2, "cpu")),
                lambda: ops.ap_hist_accum((confs, is_pos.int(), sizes, num_annos), state),
                lambda: ops.ap_hist_finalize((state[0], state[1].cpu(), state[2]))):
        with pytest.raises(L.FodError, match="ap_hist"):
            bad()
    assert int(state[1].sum()) == 0


# ---- the model ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from test_graph_gpu import _build
    return _build("bf16")[0]


def _data(seed=11):
    from future_od.datasets.synthetic import make_batch
    return make_batch(2, 3, 96, 128, seed=seed, max_boxes=9, device=DEV)


C = 8                                      # the test model's classes
SEEDS = (11, 12, 13, 14)
PREDICT = dict(top_k=300, nms=0.5)         # the launch lists
SPREAD_PREDICT = dict(top_k=2)             # the evaluators: 16 rows in all, each in a bin of its own
HEAD_SCALE, HEAD_BIAS = 16.0, -59.3172     # the class head of `spread_model`
CONTRAST = (0.25, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


@pytest.fixture(scope="module")
def spread_model():
    """The test model of test_graph_gpu.py with its class head's weights times 16 and its bias at -59.3172 (the largest
    logit of the eight clips below then sits near 0.5).  With the random weights as they are, every clip's best rows carry
    nearly one score (0.06 - 0.30, a few bins apart) and almost every (class, size) row that has candidates shares a bin;
    a trained head's scores spread over octaves, and so do these: 5e-14 .. 0.2."""
    from future_od.models.st_detr import SpatioTemporalDETRArgs
    from oracle import stdetr as O
    from runs._model import build_model
    cfg = O.Config(backbone="resnet18", enc_layers=1, dec_layers=2)
    args = SimpleNamespace(device=DEV, distributed=False, compute_dtype="bf16", backbone="resnet18")
    detr = SpatioTemporalDETRArgs(num_classes=C, num_queries=128, lr_backbone=1e-4, enc_layers=1, dec_layers=2,
                                  pretrained_backbone=False)
    net = build_model(args, detr)
    weights = O.make_state_dict(cfg, 3)
    scaled = [k for k in weights if k.endswith("class_embed.weight")]
    biases = [k for k in weights if k.endswith("class_embed.bias")]
    assert len(scaled) == len(biases) == 1
    weights[scaled[0]] = weights[scaled[0]] * HEAD_SCALE
    weights[biases[0]] = torch.full_like(weights[biases[0]], HEAD_BIAS)
    net.load_state_dict(weights)
    net.eval()
    return net


def _labelled(model, at, **options):
    """Batch `at` (0..3) and the rows `predict` returns for it.  The two clips of every batch get a contrast of their own
    (the network answers noise clips of one amplitude with nearly one set of scores).  The batch's annotations are then
    PUT on every other returned row -- the row's box shrunk about its centre by 1, 0.96, 0.92, ... (an IoU of that
    factor squared: the thresholds are crossed one after the other), its label as the class: an untrained model finds
    nothing by itself, and an AP that is 0 in every row compares nothing."""
    data = _data(SEEDS[at])
    for b in range(data["video"].shape[0]):
        data["video"][b] *= CONTRAST[2 * at + b]
    det = model.predict(data, **options)
    boxes, classes, active = (torch.zeros_like(data[k]) for k in ("boxes", "classes", "active"))
    for b in range(boxes.shape[0]):
        for i, j in enumerate(range(0, int(det["count"][b]), 2)[:9]):
            box = det["boxes"][b, j]
            centre, half = (box[:2] + box[2:]) / 2, (box[2:] - box[:2]) / 2 * (1 - 0.04 * i)
            boxes[b, i], classes[b, i], active[b, i] = torch.cat([centre - half, centre + half]), int(det["labels"][b, j]), 1
    data.update(boxes=boxes, classes=classes, active=active)
    return det, data


def _bytes(res):
    flat = {}
    for k, v in res.items():
        for k2, v2 in (v.items() if isinstance(v, dict) else [("", v)]):
            flat[k + "/" + k2] = (v2.cpu().numpy() if isinstance(v2, torch.Tensor) else np.asarray(v2)).tobytes()
    return flat


def _both_evaluators(model):
    from future_od.utils.od_map import DetectionEvaluator, StreamingDetectionEvaluator
    kept, stream = DetectionEvaluator(C), StreamingDetectionEvaluator(C)
    for at in range(len(SEEDS)):
        det, data = _labelled(model, at, **SPREAD_PREDICT)
        kept.update(det, data)
        stream.update(det, data)
    return kept, stream


def _reference_side(kept):
    """The non-streaming evaluator's tensors with the scores truncated to bf16 (what a bin is), as numpy arrays, and the
    (class, size) rows in which two candidates share a bin."""
    confs, is_pos, sizes, num_annos = (t.cpu().numpy() for t in kept.tensors())
    trunc = (confs.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    od = (trunc, is_pos.view(np.uint8), sizes.view(np.uint8), num_annos.sum(axis=2))
    return od, AC.shared_bins([od], C + 1)


def test_streaming_evaluator_against_the_evaluator_that_keeps_everything(spread_model):
    """Four batches of predict rows.  Operating point: equal integers.  Two runs: equal bytes.  The state and every
    output: the restatement's on the kept tensors, ALL rows.  AP against the sorted AP of the reference side (scores
    truncated to bf16) on the rows in which no bin is shared; the others are printed and left out."""
    from future_od.native import ops
    from future_od.utils.od_map import StreamingDetectionEvaluator, aggregate_mean_average_precision
    model = spread_model
    kept, stream = _both_evaluators(model)
    second = StreamingDetectionEvaluator(C)
    for at in reversed(range(len(SEEDS))):                   # a second run, in another order
        second.update(*_labelled(model, at, **SPREAD_PREDICT))
    assert len(stream) == 4 and len(stream._bufs) == 1 and stream.state()[0].is_cuda
    with pytest.raises(RuntimeError, match="no per-batch tensors"):
        stream.tensors()
    want, got = kept.aggregate("cpu"), stream.aggregate()
    assert _bytes(second.aggregate()) == _bytes(got)        # two runs give equal bytes
    assert set(got) == set(want) | {"coco", "pr_curve"}
    for k in ("detections", "true_positives", "annotations", "precision", "recall", "f1"):
        assert got["operating_point"][k].numpy().tobytes() == want["operating_point"][k].numpy().tobytes(), k
    assert int(got["operating_point"]["true_positives"][-1]) > 0 and int(got["operating_point"]["annotations"][-1]) > 0
    od, shared = _reference_side(kept)
    # every row, shared bins or not: the binned definition, restated on the tensors the other evaluator kept
    state = AC.restate_accum([od], 10, C + 1)
    AC.assert_results(_numpy(stream.state()), _numpy(ops.ap_hist_finalize(stream.state())),
                      dict(name="predict rows", want=state + AC.restate_finalize(*state)), "evaluator")
    print("rows (class, size) that share a bin:", np.argwhere(shared).tolist(), f"-- {shared.sum()} of {shared.size}")
    exact = AC.sorted_ap_f64(*od)
    ap = torch.cat([got["all"], got["generic"][:, None]], dim=1).numpy()
    assert ap.dtype == np.float64 and np.array_equal(np.isnan(ap), np.isnan(exact))
    assert np.nanmax(ap) > 0                                 # the annotations put on the rows are found
    keep = ~shared[None] & ~np.isnan(exact)
    n = (od[2][:, 0] != 0).sum(axis=1).max()                 # no row has more bins than its class has candidates
    f32 = aggregate_mean_average_precision(torch.from_numpy(od[0]), *(t.cpu() for t in kept.tensors()[1:]), "cpu")
    f32 = torch.cat([f32["all"], f32["generic"][:, None]], dim=1).numpy().astype(np.float64)
    assert keep.any()
    print(f"|ap - float64 sorted AP| <= {np.abs(ap - exact)[keep].max():.3e} (bound {(n + 3) * AC.U:.3e}); "
          f"|ap - float32 AP| <= {np.abs(ap - f32)[keep].max():.3e} (limit {3 * np.abs(f32 - exact)[keep].max():.3e})")
    assert np.abs(ap - exact)[keep].max() <= (n + 3) * AC.U
    assert np.abs(ap - f32)[keep].max() <= 3 * np.abs(f32 - exact)[keep].max()
    coco, curve = got["coco"]["all"].numpy(), got["pr_curve"]
    assert np.array_equal(np.isnan(coco), np.isnan(got["all"].numpy())) and np.nanmax(coco) <= 1.0 and np.nanmin(coco) >= 0.0
    assert curve["precision"].shape == (10, C + 1, 4, 101) and curve["score"].dtype == torch.float32


def test_rows_left_out_of_the_sorted_ap_comparison_are_at_most_a_tenth(spread_model):
    """The cap on the rows the test above leaves out of the comparison with the sorted AP, and that the comparison is
    about something: rows with an AP strictly inside (0, 1) are among those it keeps."""
    od, shared = _reference_side(_both_evaluators(spread_model)[0])
    print("rows (class, size) that share a bin:", np.argwhere(shared).tolist(), f"-- {shared.sum()} of {shared.size}")
    assert shared.sum() * 10 <= shared.size
    exact = AC.sorted_ap_f64(*od)
    assert ((exact > 0) & (exact < 1) & ~shared[None]).sum() >= 10


def test_launch_lists_are_what_they_were(model):
    from future_od.native import lib as L
    from future_od.utils.od_map import DetectionEvaluator, StreamingDetectionEvaluator
    data = _data()
    model.predict(data, **PREDICT)                           # (a model's first call also lays out its weights)
    L.PROFILER.start()
    det = model.predict(data, **PREDICT)
    predict = [r[0] for r in L.PROFILER.records]
    L.PROFILER.start()
    DetectionEvaluator(C).update(det, data)
    plain = [r[0] for r in L.PROFILER.records]
    stream = StreamingDetectionEvaluator(C)
    L.PROFILER.start()
    stream.update(det, data)
    stream.update(det, data)
    streaming = [r[0] for r in L.PROFILER.records]
    L.PROFILER.start()
    stream.aggregate()
    aggregate = [r[0] for r in L.PROFILER.records]
    L.PROFILER.start()
    with torch.no_grad():
        model(data=data, distributed=False)
    forward = [r[0] for r in L.PROFILER.records]
    L.PROFILER.start()
    model.predict(data, **PREDICT)
    after = [r[0] for r in L.PROFILER.records]
    L.PROFILER.stop()
    assert plain == ["fod_detect_od_map"] and streaming == ["fod_detect_od_map", "fod_ap_hist_accum"] * 2
    assert aggregate == ["fod_ap_hist_finalize"]
    assert predict == after and predict[-2:] == ["fod_detect_select", "fod_detect_nms"]
    assert not any("ap_hist" in name for name in predict + forward) and forward.count("fod_od_map") == 1


# ---- the trainer ------------------------------------------------------------------------------------------------------
class _Loader(list):
    batch_size = 2


def test_trainer_streaming_evaluation(tmp_path, capsys):
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
    tr = Trainer(net, opt, sched, _Loader(batches), {"val": _Loader(batches)}, str(tmp_path), str(tmp_path), "t", DEV,
                 print_interval=3, visualization_epochs=[], visualization_iterations=[], category_dict={}, is_master=True,
                 max_norm=detr.max_norm)
    net.to(DEV)
    plain = tr.evaluate_detections(top_k=256)["val"]
    text = capsys.readouterr().out
    assert "COCO AP" not in text and "coco" not in plain
    got = tr.set_streaming_evaluation().evaluate_detections(top_k=256)["val"]
    text = capsys.readouterr().out
    assert text.count("COCO AP") == 1 and text.count("AP50 for epoch is:") == 1 and text.count("Precision / recall") == 1
    assert set(got) == set(plain) | {"coco", "pr_curve"} and got["all"].shape == (10, 8, 4)
    for k in ("detections", "true_positives", "annotations"):
        assert torch.equal(got["operating_point"][k], plain["operating_point"][k]), k
    again = tr.set_streaming_evaluation(False).evaluate_detections(top_k=256)["val"]
    assert set(again) == set(plain) and again["all"].numpy().tobytes() == plain["all"].numpy().tobytes()
