"""AP bookkeeping over detection rows, the parts that need no GPU: the numpy restatement of tests/detect_eval_cases.py
against the CPU oracle of the existing bookkeeping where nothing is cut, ops.detect_od_map on CPU tensors against the
restatement byte for byte, padding neutrality, the hand example through DetectionEvaluator and operating_point, the entry
point as the binding reads it from include/fod_ext.h with its refusals (they return before any launch), and the
signatures that must not have moved."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import detect_eval_cases as DC
from future_od.native import abi
from oracle import od_map as OM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, FL = "pointer", "int", "float"
ENTRY = "fod_detect_od_map"
CASES = DC.all_cases()
IDS = [c["name"] for c in CASES]
GROUP1 = [c for c in CASES if c["name"].startswith("all-pairs")]


def _tensors(case):
    return tuple(torch.from_numpy(case[k].copy()) for k in DC.ROWS + DC.ANNOS)


def _run(case, **kw):
    from future_od.native import ops
    return ops.detect_od_map(*_tensors(case), case["imsize"], case["C"], case["per_class"], T=case["T"], **kw)


def _assert_equal(got, case, what):
    for name, g, w in zip(DC.OUTS, got, case["want"]):
        g = g.numpy()
        g = g.view(np.uint8) if g.dtype == np.bool_ else g
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (what, case["name"], name, g, w)


# ---- the restatement against the existing bookkeeping ------------------------------------------------------------------
@pytest.mark.parametrize("case", GROUP1, ids=[c["name"] for c in GROUP1])
def test_restatement_equals_the_oracle_of_od_map_when_nothing_is_cut(case):
    confs, is_pos, sizes, num_annos = OM.prepare_od_map_stuffs(case["px"], case["dense"], case["anno_boxes"],
                                                               case["anno_classes"], case["anno_active"], case["imsize"])
    want = case["want"]
    assert confs.shape == want[0].shape and confs.dtype == want[0].dtype
    assert np.array_equal(confs, want[0]) and np.array_equal(is_pos, want[1].astype(bool))
    assert np.array_equal(sizes, want[2].astype(bool)) and np.array_equal(num_annos, want[3])


def test_group_1_has_the_sizes_and_the_tie():
    assert [(c["logits"].shape[0],) + c["logits"].shape[1:] + (c["anno_boxes"].shape[1],) for c in GROUP1] == \
        [(B, M, C, N) for B, M, C, N in DC.GROUP1_SIZES]
    for c in GROUP1:
        B, M, C = c["logits"].shape
        assert c["scores"].shape[1] == M * C and c["P"] == min(50, M) and c["scores"][0, 0] == c["scores"][0, 1]


# ---- the CPU form against the restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cpu_form_equals_the_restatement(case):
    inputs = _tensors(case)
    before = [t.clone() for t in inputs]
    from future_od.native import ops
    got = ops.detect_od_map(*inputs, case["imsize"], case["C"], case["per_class"], T=case["T"])
    assert got[1].dtype == got[2].dtype == torch.bool
    _assert_equal(got, case, "fresh outputs")
    for t, b in zip(inputs, before):                       # the inputs are untouched (bytes: NaN rows compare too)
        assert t.numpy().tobytes() == b.numpy().tobytes()
    out = (torch.full_like(got[0], 7.5), torch.full(got[1].shape, 77, dtype=torch.uint8),
           torch.full(got[2].shape, 77, dtype=torch.uint8), torch.full_like(got[3], 77))
    again = ops.detect_od_map(*inputs, case["imsize"], case["C"], case["per_class"], T=case["T"], out=out)
    assert all(a is o for a, o in zip(again, out))
    _assert_equal(again, case, "given outputs")


def test_garbage_beyond_count_is_never_read():
    case = next(c for c in CASES if c["name"] == "cut-count-0-in-the-middle")
    hostile = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}
    B, K = case["scores"].shape
    for b in range(B):
        n = min(max(int(case["count"][b]), 0), K)
        hostile["boxes"][b, n:] = hostile["anno_boxes"][b, 0]          # would claim an annotation
        hostile["boxes"][b, n + 1:] = np.nan
        hostile["labels"][b, n:] = 0
        hostile["query"][b, n:] = 4242
        hostile["scores"][b, n:] = 9.0
    _assert_equal(_run(hostile), case, "hostile tail")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_padding_slots_are_neutral_in_the_ap(case):
    """The reference's AP sorts the slots by confs: wherever a padding slot sorts, it adds to no cumulative sum.  With the
    padding's confs at 5.0 (in front of everything) instead of 0:
    - the TERMS of the AP -- the precision at every true positive, in rank order, by average_precision's own formula -- are
      the same bytes;
    - oracle.od_map.average_precision itself is unchanged up to the ORDER of its float32 sum: numpy adds the P products
      pairwise by position, and the zeros of the padding sit at other positions, so the last bit may differ (it does on
      three of the cases: one ulp).  The bound is that of a float32 sum of at most P non-negative terms in any order,
      (P - 1) * 2^-24 relative; where there is no padding the two are the same bytes."""
    confs, is_pos, sizes, num_annos = case["want"]
    pad = sizes[:, 0] == 0
    moved = confs.copy()
    moved[:, pad] = 5.0
    slots = confs.shape[2]

    def terms(cf, t):
        out = []
        for c in range(cf.shape[1]):
            ids = np.argsort(-cf[t, c], kind="stable")
            for s in range(4):
                pos = (is_pos[t, c].astype(bool) & sizes[c, s].astype(bool))[ids]
                cnt = sizes[c, s].astype(bool)[ids]
                prec = np.cumsum(pos).astype(np.float32) / (np.cumsum(cnt).astype(np.float32) + np.float32(1e-5))
                out.append(prec[pos].tobytes())
        return out

    for t in (0, case["T"] - 1):
        assert terms(confs, t) == terms(moved, t), (case["name"], t)
        with np.errstate(all="ignore"):
            a = OM.average_precision(confs[t], is_pos[t].astype(bool), sizes.astype(bool), num_annos[:, :, None])
            b = OM.average_precision(moved[t], is_pos[t].astype(bool), sizes.astype(bool), num_annos[:, :, None])
        if not pad.any():
            assert a.tobytes() == b.tobytes(), (case["name"], t)
        ok = np.isfinite(a)                                  # (a class without annotations: x / 0)
        assert np.array_equal(ok, np.isfinite(b)) and np.array_equal(a[~ok], b[~ok], equal_nan=True), (case["name"], t)
        assert (np.abs(a[ok].astype(np.float64) - b[ok]) <= (slots - 1) * 2.0 ** -24 * np.maximum(a[ok], b[ok])).all(), \
            (case["name"], t, a, b)
    assert not (is_pos[:, pad] != 0).any() and not (confs[:, pad] != 0).any()
    assert not any((sizes[:, k][pad] != 0).any() for k in range(4))


def test_some_case_has_padding_that_would_sort_first():
    assert sum(int((c["want"][2][:, 0] == 0).sum()) > 0 for c in CASES) >= 8


# ---- the hand example -----------------------------------------------------------------------------------------------------
def _evaluate(case):
    from future_od.utils.od_map import DetectionEvaluator
    rows = _tensors(case)
    det = dict(zip(DC.ROWS, rows[:5]))
    H, W = case["imsize"]
    data = {"boxes": rows[5], "classes": rows[6], "active": rows[7], "video": torch.zeros(1, 1, 3, H, W)}
    ev = DetectionEvaluator(case["C"])
    od = ev.update(det, data)
    _assert_equal(od, case, "evaluator")
    return ev, od


def test_hand_example_ap_with_and_without_suppression(capsys):
    plain, nms = DC.hand()
    for case, want in zip((plain, nms), DC.HAND_AP50):
        ev, _ = _evaluate(case)
        ap = ev.aggregate("cpu")
        assert set(ap) == {"all", "classavg", "threshavg", "classavg threshavg", "generic", "generic threshavg",
                           "operating_point"}
        assert ap["all"].shape == (10, 1, 4) and ap["generic"].shape == (10, 4)
        assert abs(float(ap["all"][0, 0, 0]) - want) < 1e-4, (case["name"], float(ap["all"][0, 0, 0]), want)
        assert abs(float(ap["generic"][0, 0]) - want) < 1e-4
    assert abs(DC.HAND_AP50[0] - 5 / 6) < 1e-12 and DC.HAND_AP50[1] == 1.0
    # two updates concatenate as the trainer's epoch does: twice the same batch is the same AP
    ev, _ = _evaluate(plain)
    ev.update(dict(zip(DC.ROWS, _tensors(plain)[:5])), {"boxes": _tensors(plain)[5], "classes": _tensors(plain)[6],
                                                        "active": _tensors(plain)[7], "video": torch.zeros(1, 1, 3, 96, 128)})
    assert len(ev) == 2 and [t.shape[2] for t in ev.tensors()] == [6, 6, 6, 2]
    ev.aggregate("cpu")
    ev.reset()
    with pytest.raises(RuntimeError, match="no update"):
        ev.aggregate()


def test_operating_point_on_the_hand_example():
    from future_od.utils.od_map import operating_point
    plain, nms = DC.hand()
    for case, (det, tp) in zip((plain, nms), ((3, 2), (2, 2))):
        ev, od = _evaluate(case)
        for op in (operating_point(*od), ev.aggregate("cpu")["operating_point"]):
            assert op["iou"] == 0.5
            for k in ("detections", "true_positives", "annotations"):
                assert op[k].dtype == torch.int64 and op[k].shape == (2,)          # the class and the generic class
            assert op["detections"].tolist() == [det, det] and op["true_positives"].tolist() == [tp, tp]
            assert op["annotations"].tolist() == [2, 2]
            assert op["precision"].tolist() == [tp / det] * 2 and op["recall"].tolist() == [1.0, 1.0]
            assert op["f1"].tolist() == [2 * tp / (det + 2)] * 2
    # a stricter threshold: the shifted copy aside, the rows are exact boxes -- nothing changes at IoU 0.95
    assert operating_point(*_evaluate(plain)[1], t=9)["true_positives"].tolist() == [2, 2]
    # a class without detections or annotations: NaN, not a division error
    z = operating_point(torch.zeros(10, 1, 4), torch.zeros(10, 1, 4, dtype=torch.bool), torch.zeros(1, 4, 4, dtype=torch.bool),
                        torch.zeros(1, 4, dtype=torch.int64))
    assert all(np.isnan(z[k].tolist()[0]) for k in ("precision", "recall", "f1")) and z["detections"].tolist() == [0]


def test_detections_through_a_box_map_are_refused():
    from future_od.utils.od_map import DetectionEvaluator, prepare_od_map_detections
    case = DC.hand()[0]
    rows = _tensors(case)
    det = dict(zip(DC.ROWS, rows[:5]))
    with pytest.raises(ValueError, match="box_map"):
        prepare_od_map_detections(dict(det, box_map=torch.ones(1, 4)), rows[5], rows[6], rows[7], case["imsize"], 1)
    data = {"boxes": rows[5], "classes": rows[6], "active": rows[7], "video": torch.zeros(1, 1, 3, 96, 128),
            "box_map": torch.ones(1, 4)}
    with pytest.raises(ValueError, match="box_map"):
        DetectionEvaluator(1).update(det, data)
    got = prepare_od_map_detections(det, rows[5], rows[6], rows[7], case["imsize"], 1)
    _assert_equal(got, case, "prepare_od_map_detections")


# ---- ABI and binding ---------------------------------------------------------------------------------------------------
def test_entry_is_bound_with_the_headers_signature_and_the_abi_moved():
    from future_od.native import lib as L
    hdr = open(os.path.join(ROOT, "include", "fod.h")).read()
    assert int(re.search(r"#define FOD_ABI_VERSION (\d+)", hdr).group(1)) == L.ABI_VERSION == L.LIB.fod_abi_version() >= 18
    assert abi.EXT_PROTOTYPES[ENTRY] == (I, [P] * 12 + [I] * 6 + [FL, FL, P])
    assert ENTRY not in abi.PROTOTYPES and ENTRY not in hdr and ENTRY in L.EXT_SIGNATURES
    ext = open(os.path.join(ROOT, "include", "fod_ext.h")).read()
    proto = re.search(r"\bint\s+fod_detect_od_map\s*\(([^;]*)\);", ext).group(1)
    assert len(proto.split(",")) == len(L.EXT_SIGNATURES[ENTRY]) == 21
    fn = getattr(L.LIB, ENTRY)
    assert fn.restype is abi.CTYPE[I] and list(fn.argtypes) == [abi.CTYPE[k] for k in abi.EXT_PROTOTYPES[ENTRY][1]]
    assert "detect_eval" in open(os.path.join(ROOT, "future-object-detection_amd", "build.sh")).read()


def _entry(B=1, K=4, N=3, C=2, P_=2, T=10, null=()):
    """The non-null 'pointers' are the address 8: a launch would fault, so a clean non-zero return is the check itself.
    Operands 0..7 are the inputs, 8..11 the outputs."""
    from future_od.native import lib as L
    p = [None if k in null else 8 for k in range(12)]
    rc = getattr(L.LIB, ENTRY)(*p, B, K, N, C, P_, T, 96.0, 128.0, None)
    return rc, L.last_error()


@pytest.mark.parametrize("kw, texts", [
    (dict(B=0), ("B=0", "at least 1")), (dict(B=-2), ("B=-2", "at least 1")),
    (dict(K=0), ("K=0", "1..1024")), (dict(K=1025, P_=2), ("K=1025", "1..1024")), (dict(K=-1), ("K=-1", "1..1024")),
    (dict(N=0), ("N=0", "1..1024")), (dict(N=1025), ("N=1025", "1..1024")),
    (dict(P_=0), ("P=0", "1..K=4")), (dict(P_=5), ("P=5", "1..K=4")), (dict(P_=-1), ("P=-1", "1..K=4")),
    (dict(T=0), ("T=0", "1..16")), (dict(T=17), ("T=17", "1..16")),
    (dict(C=0), ("C=0", "at least 1")), (dict(C=-1), ("C=-1", "at least 1")),
] + [(dict(null=(k,)), ("null operand",)) for k in range(12)])
def test_arguments_are_refused_before_any_launch(kw, texts):
    from future_od.native import lib as L
    rc, err = _entry(**kw)
    assert rc == L.ERR_ARG and err.startswith("detect_od_map:") and all(t in err for t in texts), (kw, rc, err)


def test_wrapper_refuses_bad_operands():
    from future_od.native import lib as L
    from future_od.native import ops
    case = CASES[0]
    s, l, b, q, c, ab, ac, aa = _tensors(case)
    im, C = case["imsize"], case["C"]
    run = lambda *a, **kw: (lambda: ops.detect_od_map(*a, **kw))
    big = 1025
    for bad in (run(s.double(), l, b, q, c, ab, ac, aa, im, C), run(s, l.long(), b, q, c, ab, ac, aa, im, C),
                run(s, l, b[:, :, :3], q, c, ab, ac, aa, im, C), run(s, l, b, q[:, :2], c, ab, ac, aa, im, C),
                run(s, l, b, q, c.long(), ab, ac, aa, im, C), run(s[0], l, b, q, c, ab, ac, aa, im, C),
                run(s, l, b, q, c, ab[:, :, :3], ac, aa, im, C), run(s, l, b, q, c, ab, ac.int(), aa, im, C),
                run(s, l, b, q, c, ab, ac, aa[:, :2], im, C), run(s, l, b, q, c, ab, ac, aa.bool(), im, C),
                run(s, l, b.transpose(1, 2).contiguous().transpose(1, 2), q, c, ab, ac, aa, im, C),
                run(s, l, b, q, c, ab, ac, aa, im, 0), run(s, l, b, q, c, ab, ac, aa, im, C, per_class=0),
                run(s, l, b, q, c, ab, ac, aa, im, C, T=0), run(s, l, b, q, c, ab, ac, aa, im, C, T=17),
                run(s, l, b, q, c, ab, ac, aa, im, C, out=(s, l, b)),
                run(s, l, b, q, c, ab, ac, aa, im, C, out=tuple(torch.zeros(1) for _ in range(4))),
                run(torch.zeros(1, big), torch.zeros(1, big, dtype=torch.int32), torch.zeros(1, big, 4),
                    torch.zeros(1, big, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), ab[:1], ac[:1], aa[:1], im, C),
                run(s[:1], l[:1], b[:1], q[:1], c[:1], torch.zeros(1, big, 4), torch.zeros(1, big, dtype=torch.int64),
                    torch.zeros(1, big, dtype=torch.int64), im, C)):
        with pytest.raises(L.FodError, match="detect_od_map"):
            bad()
    # per_class above the number of rows is not an error: P = min(per_class, K)
    small = ops.detect_od_map(s[:, :9].contiguous(), l[:, :9].contiguous(), b[:, :9].contiguous(), q[:, :9].contiguous(),
                              torch.full_like(c, 9), ab, ac, aa, im, C)
    assert small[0].shape == (10, C + 1, s.shape[0] * 9)


# ---- nothing else moved ----------------------------------------------------------------------------------------------------
def test_signatures_are_what_they_were():
    from future_od.graph import GraphedPredict
    from future_od.models.st_detr import SpatioTemporalDETR
    from future_od.trainer import Trainer
    from future_od.utils import od_map
    sig = inspect.signature(SpatioTemporalDETR.predict).parameters
    assert list(sig) == ["self", "data", "top_k", "score_threshold", "per_query", "box_map", "attention", "nms",
                         "nms_class_agnostic"]
    assert [sig[k].default for k in list(sig)[2:]] == [100, 0.0, False, None, False, None, False]
    sig = inspect.signature(GraphedPredict.__init__).parameters
    assert list(sig) == ["self", "model", "top_k", "score_threshold", "per_query", "warmup", "attention", "nms",
                         "nms_class_agnostic"]
    assert [sig[k].default for k in list(sig)[2:]] == [100, 0.0, False, 1, False, None, False]
    sig = inspect.signature(Trainer.__init__).parameters
    assert list(sig) == ["self", "model", "optimizer", "lr_sched", "train_loader", "val_loaders", "checkpoint_path",
                         "visualization_path", "save_name", "device", "print_interval", "visualization_epochs",
                         "visualization_iterations", "category_dict", "checkpoint_epochs", "gradient_clip_value",
                         "distributed", "is_master", "wandb_config", "max_norm", "ema"]
    sig = inspect.signature(Trainer.evaluate_detections).parameters
    assert list(sig) == ["self", "top_k", "score_threshold", "per_query", "nms", "nms_class_agnostic", "per_class"]
    assert [sig[k].default for k in list(sig)[1:]] == [100, 0.0, False, None, False, 50]
    sig = inspect.signature(od_map.prepare_od_map_detections).parameters
    assert list(sig) == ["det", "anno_boxes", "anno_classes", "anno_active", "imsize", "num_classes", "per_class"]
    assert list(inspect.signature(od_map.prepare_od_map_stuffs).parameters) == \
        ["pred_boxes", "pred_class_scores", "anno_boxes", "anno_classes", "anno_active", "imsize"]
    sig = inspect.signature(od_map.DetectionEvaluator.__init__).parameters
    assert list(sig) == ["self", "num_classes", "per_class"] and sig["per_class"].default == 50


def test_more_than_one_rank_is_refused(monkeypatch):
    import torch.distributed as distrib
    from future_od.trainer import Trainer
    tr = Trainer.__new__(Trainer)
    tr._distributed = True
    monkeypatch.setattr(distrib, "is_initialized", lambda: True)
    monkeypatch.setattr(distrib, "get_world_size", lambda *a: 2)
    with pytest.raises(NotImplementedError, match="ranks"):
        tr.evaluate_detections()
