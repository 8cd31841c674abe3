"""Label-free inference, the parts that need no GPU: the fod_detect_select binding and its argument checks (they return
before any launch), Plan.box_map() against Plan.annotate, and the label-free form of DeviceJointTransform.host."""
import os
import random
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANNOTATION_KEYS = ("boxes", "classes", "active", "ignore_boxes", "annotated_frame_idx")


def test_detect_select_is_bound_and_the_abi_moved():
    from future_od.native import lib as L
    assert "fod_detect_select" in L.FAST and "fod_detect_select" in L.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "fod.h")).read()
    assert int(re.search(r"#define FOD_ABI_VERSION (\d+)", hdr).group(1)) == L.ABI_VERSION == L.LIB.fod_abi_version() >= 9
    proto = re.search(r"fod_detect_select\s*\(([^;]*)\);", hdr).group(1)
    assert len(proto.split(",")) == len(L.SIGNATURES["fod_detect_select"]) == 17


def _select_args(B=1, M=4, C=3, K=2, per_query=0, null=False):
    """Arguments of fod_detect_select over host buffers: every case below is refused before anything is launched, so no
    pointer is ever read."""
    buf = torch.zeros(16)
    p = None if null else buf.data_ptr()
    return buf, (p, p, None, B, M, C, K, 0.0, per_query, 96.0, 128.0, p, p, p, p, p, None)


@pytest.mark.parametrize("entry", ["ctypes", "fastcall"])
@pytest.mark.parametrize("kwargs,names", [
    (dict(null=True), ("null",)),
    (dict(K=0), ("K=0", "1..1024")),
    (dict(K=1025), ("K=1025", "1..1024")),
    (dict(M=8193, C=1, per_query=0), ("8193", "M*C", "8192")),
    (dict(M=8193, C=2, per_query=1), ("8193", "8192")),
    (dict(M=4097, C=2, per_query=0), ("8194", "M*C", "8192")),
])
def test_detect_select_argument_checks_name_the_limit(entry, kwargs, names):
    from future_od.native import lib as L
    fn = L.LIB.fod_detect_select if entry == "ctypes" else L.FAST["fod_detect_select"]
    keep, args = _select_args(**kwargs)
    assert fn(*args) == 1                                   # FOD_ERR_ARG
    msg = L.last_error()
    assert msg.startswith("detect_select:") and all(n in msg for n in names), msg
    del keep


def test_detect_select_has_no_cpu_fallback():
    from future_od.native import lib as L
    from future_od.native import ops
    with pytest.raises(L.FodError, match="device tensor"):
        ops.detect_select(torch.zeros(1, 4, 3), torch.zeros(1, 4, 4), 96, 128, 2)


def test_box_map_inverts_annotate():
    """300 plans of RandomSizedCrop(0.5, 1.0) -> JointResize((448, 800)) on a 900 x 1600 frame, every second one followed
    by a flip; 20 boxes per plan strictly inside the crop rectangle, wider and taller than 1 px.  annotate() followed by
    the map (in f32, as the kernel applies it) with the corners re-ordered gives the source boxes back within 2e-3 px:
    a few f32 roundings at 1600 px (2^-13 = 1.2e-4 each)."""
    import future_od.datasets.transforms as T
    h0, w0 = 900, 1600
    crop, resize = T.RandomSizedCrop(0.5, 1.0), T.JointResize((448, 800))
    g = torch.Generator().manual_seed(7)
    worst, flips, total = 0.0, 0, 0
    for i in range(300):
        steps = [crop, resize] + ([T.JointHorizontalFlip(1.0)] if i % 2 else [])
        plan = T.JointCompose(steps).plan(h0, w0, random.Random(1000 + i))
        top, left, h, w = plan.rect
        assert plan.size == (448, 800) and plan.flip == bool(i % 2)
        u = torch.rand(20, 4, generator=g, dtype=torch.float64)
        x0 = left + 0.5 + u[:, 0] * (w - 3)
        y0 = top + 0.5 + u[:, 1] * (h - 3)
        x1 = x0 + 1.01 + u[:, 2] * ((left + w - 0.5) - x0 - 1.01)
        y1 = y0 + 1.01 + u[:, 3] * ((top + h - 0.5) - y0 - 1.01)
        src = torch.stack([x0, y0, x1, y1], dim=1).float()
        assert bool((src[:, 0] > left).all() and (src[:, 2] < left + w).all() and (src[:, 1] > top).all()
                    and (src[:, 3] < top + h).all() and (src[:, 2] - src[:, 0] > 1).all() and (src[:, 3] - src[:, 1] > 1).all())
        out, cls = plan.annotate(src, torch.zeros(20, dtype=torch.int64))
        assert out.shape == (20, 4)                                  # nothing inside the rectangle is dropped
        sx, sy, ox, oy = (torch.tensor(v, dtype=torch.float32) for v in plan.box_map())
        assert (float(sx) < 0) == plan.flip
        xa, xb, ya, yb = out[:, 0] * sx + ox, out[:, 2] * sx + ox, out[:, 1] * sy + oy, out[:, 3] * sy + oy
        back = torch.stack([torch.minimum(xa, xb), torch.minimum(ya, yb), torch.maximum(xa, xb), torch.maximum(ya, yb)], dim=1)
        worst = max(worst, float((back.double() - src.double()).abs().max()))
        flips += plan.flip
        total += 20
    print(f"box_map round trip: {total} boxes, {flips} flipped plans, worst error {worst:.3e} px")
    assert flips == 150 and total == 6000
    assert worst <= 2e-3, worst
    # the closed forms
    plan = T.JointCompose([T.JointCenterCrop((96, 128))]).plan(120, 160)
    assert plan.box_map() == (1.0, 1.0, 16.0, 12.0)
    plan = T.JointCompose([T.JointCenterCrop((96, 128)), T.JointResize((48, 32)), T.JointHorizontalFlip(1.0)]).plan(120, 160)
    assert plan.box_map() == (-4.0, 2.0, 144.0, 12.0)


def _label_free(batch):
    return {k: v for k, v in batch.items() if k not in ANNOTATION_KEYS + ("_host_annotations",)}


def test_device_transform_host_half_on_label_free_batches():
    import future_od.datasets.transforms as T
    from future_od.datasets.synthetic import make_batch
    from future_od.utils.augment import DeviceJointTransform
    t = T.JointCompose([T.RandomSizedCrop(0.5, 0.9), T.JointResize((64, 96)), T.JointHorizontalFlip(0.5)])
    labelled = make_batch(4, 2, 90, 160, seed=21, max_boxes=9, raw_frames=True)
    free = _label_free(labelled)
    assert not set(free) & set(ANNOTATION_KEYS)
    flips = 0
    for index in range(3):
        out = DeviceJointTransform(t, seed=5, rank=0).host(free, index=index)
        assert set(out) == set(free) | {"plans", "_plan_size", "box_map"}          # no annotation keys, no host copies
        assert out["video"] is free["video"] and out["_plan_size"] == (64, 96)
        assert out["box_map"].dtype == torch.float32 and out["box_map"].shape == (4, 4)
        dt = DeviceJointTransform(t, seed=5, rank=0)
        for b in range(4):
            plan = t.plan(90, 160, dt.sample_rng(index, b))
            assert out["plans"][b].tolist() == list(plan.row())
            assert torch.equal(out["box_map"][b], torch.tensor(plan.box_map(), dtype=torch.float32))
            flips += plan.flip
        # the labelled batch draws the same plans and keeps today's keys and values: nothing about a map
        lab = DeviceJointTransform(t, seed=5, rank=0).host(labelled, index=index)
        assert set(lab) == set(labelled) | {"plans", "_plan_size"} and "box_map" not in lab
        assert torch.equal(lab["plans"], out["plans"])
        for b in range(4):
            rows = labelled["active"][b].bool()
            bx, cl = t.plan(90, 160, dt.sample_rng(index, b)).annotate(labelled["boxes"][b][rows], labelled["classes"][b][rows])
            n = bx.shape[0]
            assert torch.equal(lab["boxes"][b, :n], bx) and torch.equal(lab["classes"][b, :n], cl)
            assert int(lab["active"][b].sum()) == n and not lab["boxes"][b, n:].any()
        assert set(lab["_host_annotations"]) == {"active", "boxes", "classes"}
    assert 0 < flips < 12
    for missing in ("boxes", "classes", "active"):
        partial = {k: v for k, v in labelled.items() if k != missing}
        with pytest.raises(ValueError, match="all of boxes / classes / active or none"):
            DeviceJointTransform(t).host(partial)


def test_predict_reads_no_annotation_and_refuses_train_mode():
    """predict() on a stand-in core: the keys it hands to GraphedPredict are the ones it reads, and train mode is
    refused before anything runs (the device path is covered by tests/test_predict_gpu.py)."""
    from future_od.datasets.synthetic import make_batch
    from future_od.models.st_detr import SpatioTemporalDETR, SpatioTemporalDETRArgs
    model = SpatioTemporalDETR(SpatioTemporalDETRArgs(num_classes=8, encode_offset=True), torch.nn.Identity())
    data = _label_free(make_batch(1, 2, 16, 24, seed=3))
    assert set(model.predict_inputs(data)) == {"video", "translation", "acceleration", "rotation", "rotation_rate", "speed",
                                               "temporal_offsets"}
    data["box_map"] = torch.zeros(1, 4)
    assert "box_map" in model.predict_inputs(data)
    assert set(model.predict_inputs({"video": data["video"], "temporal_offsets": data["temporal_offsets"],
                                     "boxes": torch.zeros(1, 2, 4)})) == {"video", "temporal_offsets"}
    model.train()
    with pytest.raises(RuntimeError, match="evaluation only"):
        model.predict(data)
