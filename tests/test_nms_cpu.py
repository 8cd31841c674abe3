"""Duplicate suppression, the parts that need no GPU: fod_detect_nms as the binding reads it from include/fod_ext.h and its
argument checks (they return before any launch), ops.detect_nms on CPU tensors against the numpy restatement of
tests/nms_cases.py byte for byte, the conditioning of the random cases, and the new keywords of predict / GraphedPredict."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import nms_cases as NC
from future_od.native import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, FL = "pointer", "int", "float"
ENTRY = "fod_detect_nms"
CASES = NC.all_cases()
IDS = [c["name"] for c in CASES]


# ---- ABI and binding ---------------------------------------------------------------------------------------------------
def test_entry_is_bound_with_the_headers_signature_and_the_abi_moved():
    from future_od.native import lib as L
    hdr = open(os.path.join(ROOT, "include", "fod.h")).read()
    assert int(re.search(r"#define FOD_ABI_VERSION (\d+)", hdr).group(1)) == L.ABI_VERSION == L.LIB.fod_abi_version() >= 17
    assert abi.EXT_PROTOTYPES[ENTRY] == (I, [P, P, P, P, P, I, I, FL, I, P, P, P, P, P, P, P])
    assert ENTRY not in abi.PROTOTYPES and ENTRY not in hdr
    ext = open(os.path.join(ROOT, "include", "fod_ext.h")).read()
    proto = re.search(r"\bint\s+fod_detect_nms\s*\(([^;]*)\);", ext).group(1)
    assert len(proto.split(",")) == len(L.EXT_SIGNATURES[ENTRY]) == 16
    fn = getattr(L.LIB, ENTRY)
    assert fn.restype is abi.CTYPE[I] and list(fn.argtypes) == [abi.CTYPE[k] for k in abi.EXT_PROTOTYPES[ENTRY][1]]


def _entry(B=1, K=4, thr=0.5, agnostic=0, null=(), source=1):
    """The non-null 'pointers' are the address 1: a launch would fault, so a clean non-zero return is the check itself.
    Operands 0..4 are the inputs, 5..9 the outputs."""
    from future_od.native import lib as L
    p = [None if k in null else 1 for k in range(10)]
    rc = getattr(L.LIB, ENTRY)(*p[:5], B, K, thr, agnostic, *p[5:], source, None)
    return rc, L.last_error()


@pytest.mark.parametrize("kw, texts", [
    (dict(K=0), ("K=0", "1..1024")), (dict(K=1025), ("K=1025", "1..1024")), (dict(K=-1), ("K=-1", "1..1024")),
    (dict(B=0), ("B=0", "at least 1")), (dict(B=-2), ("B=-2", "at least 1")),
    (dict(thr=-0.01), ("iou_threshold", "[0, 1]")), (dict(thr=1.5), ("iou_threshold", "[0, 1]")),
    (dict(thr=float("nan")), ("iou_threshold", "[0, 1]")), (dict(thr=float("inf")), ("iou_threshold", "[0, 1]")),
    (dict(thr=float("-inf")), ("iou_threshold", "[0, 1]")),
] + [(dict(null=(k,)), ("null operand",)) for k in range(10)])
def test_arguments_are_refused_before_any_launch(kw, texts):
    from future_od.native import lib as L
    rc, err = _entry(**kw)
    assert rc == L.ERR_ARG and err.startswith("detect_nms:") and all(t in err for t in texts), (kw, rc, err)


def test_every_limit_is_checked_with_a_null_source_too():
    from future_od.native import lib as L
    rc, err = _entry(K=1025, source=None)
    assert rc == L.ERR_ARG and "1..1024" in err


# ---- the CPU form against the restatement --------------------------------------------------------------------------------
def _tensors(case):
    return tuple(torch.from_numpy(case[k].copy()) for k in NC.NAMES[:5])


def _assert_equal(got, case, what):
    for name, g, w in zip(NC.NAMES, got, case["want"]):
        g = g.numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        assert g.tobytes() == w.tobytes(), (what, case["name"], name, g, w)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cpu_form_equals_the_restatement(case):
    from future_od.native import ops
    inputs = _tensors(case)
    before = [t.clone() for t in inputs]
    got = ops.detect_nms(*inputs, case["thr"], case["agnostic"])
    assert len(got) == 6
    _assert_equal(got, case, "fresh outputs")
    for t, b in zip(inputs, before):                       # the inputs are untouched (bytes: NaN rows compare too)
        assert t.numpy().tobytes() == b.numpy().tobytes()
    # in place: the outputs are the inputs
    source = torch.full(inputs[1].shape, 77, dtype=torch.int32)
    again = ops.detect_nms(*inputs, case["thr"], case["agnostic"], out=inputs + (source,))
    assert all(a is o for a, o in zip(again, inputs + (source,)))
    _assert_equal(again, case, "in place")


def test_cpu_form_refuses_bad_operands():
    from future_od.native import lib as L
    from future_od.native import ops
    s, l, b, q, c = _tensors(CASES[0])
    for bad in (lambda: ops.detect_nms(s, l, b, q, c, 1.5), lambda: ops.detect_nms(s, l, b, q, c, float("nan")),
                lambda: ops.detect_nms(s, l, b, q, c, -0.1),
                lambda: ops.detect_nms(s.double(), l, b, q, c), lambda: ops.detect_nms(s, l.long(), b, q, c),
                lambda: ops.detect_nms(s, l, b[:, :, :3], q, c), lambda: ops.detect_nms(s, l, b, q[:, :2], c),
                lambda: ops.detect_nms(s, l, b, q, c.long()), lambda: ops.detect_nms(s[0], l, b, q, c),
                lambda: ops.detect_nms(s, l, b.transpose(1, 2).contiguous().transpose(1, 2), q, c),
                lambda: ops.detect_nms(s, l, b, q, c, out=(s, l, b, q, c)),
                lambda: ops.detect_nms(s, l, b, q, c, out=(s, l, b, q, c, torch.zeros(s.shape))),
                lambda: ops.detect_nms(torch.zeros(1, 1025), torch.zeros(1, 1025, dtype=torch.int32), torch.zeros(1, 1025, 4),
                                       torch.zeros(1, 1025, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))):
        with pytest.raises(L.FodError, match="detect_nms"):
            bad()


# ---- conditioning of the random cases ------------------------------------------------------------------------------------
def test_random_cases_are_decided_alike_by_a_float64_division():
    """A condition on the INPUTS, not a tolerance: on the committed seeds no pair the restatement evaluates sits so close
    to its threshold that a float64 `inter / uni > thr` would decide it the other way."""
    evaluated = 0
    for case in CASES:
        if case["name"].startswith("random"):
            bad, total = NC.f64_disagreements(case)
            assert bad == 0, (case["name"], bad, total)
            evaluated += total
    print(f"random cases: {evaluated} pairs evaluated, 0 decided differently in float64")
    assert evaluated > 100000


def test_random_cases_cover_the_shapes():
    names = [c["name"] for c in CASES if c["name"].startswith("random") and not c["name"].endswith("tail")]
    for K in NC.RANDOM_KS:
        assert sum(f"-K{K}-" in n for n in names) >= 2
    for thr in NC.THRESHOLDS:
        assert any(f"-thr{thr}-" in n for n in names)
    assert any(n.endswith("agnostic") for n in names) and any("labels1" in n for n in names) and any("labels9" in n for n in names)
    assert sum(c["name"].endswith("garbage-tail") for c in CASES) >= 10


# ---- predict / GraphedPredict ----------------------------------------------------------------------------------------------
def test_predict_with_nms_refuses_train_mode():
    from future_od.datasets.synthetic import make_batch
    from future_od.models.st_detr import SpatioTemporalDETR, SpatioTemporalDETRArgs
    model = SpatioTemporalDETR(SpatioTemporalDETRArgs(num_classes=8, encode_offset=True), torch.nn.Identity())
    data = make_batch(1, 2, 16, 24, seed=3)
    model.train()
    with pytest.raises(RuntimeError, match="evaluation only"):
        model.predict(data, nms=0.5)
    with pytest.raises(RuntimeError, match="evaluation only"):
        model.predict(data, nms=0.5, nms_class_agnostic=True)


def test_old_parameters_keep_their_order_and_the_new_ones_follow():
    from future_od.graph import GraphedPredict
    from future_od.models.st_detr import SpatioTemporalDETR
    sig = inspect.signature(SpatioTemporalDETR.predict).parameters
    assert list(sig) == ["self", "data", "top_k", "score_threshold", "per_query", "box_map", "attention", "nms",
                         "nms_class_agnostic"]
    assert [sig[k].default for k in list(sig)[2:]] == [100, 0.0, False, None, False, None, False]
    assert all(sig[k].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for k in list(sig)[:7])
    sig = inspect.signature(GraphedPredict.__init__).parameters
    assert list(sig) == ["self", "model", "top_k", "score_threshold", "per_query", "warmup", "attention", "nms",
                         "nms_class_agnostic"]
    assert [sig[k].default for k in list(sig)[2:]] == [100, 0.0, False, 1, False, None, False]
    assert all(sig[k].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for k in list(sig)[:7])
    gp = GraphedPredict(torch.nn.Identity(), 50, 0.1, True, 2, True, nms=0.25, nms_class_agnostic=True)
    assert (gp.top_k, gp.score_threshold, gp.per_query, gp.warmup, gp.attention) == (50, 0.1, True, 2, True)
    assert (gp.nms, gp.nms_class_agnostic) == (0.25, True) and GraphedPredict(torch.nn.Identity()).nms is None
