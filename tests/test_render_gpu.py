"""fod_render_boxes on the device: every case of tests/render_cases.py against the numpy restatement byte for byte (f32
and uint8 sources, aligned and unaligned destinations, a guard band behind the picture), `out=` reuse, a side stream,
render_detections, a captured launch replayed after its boxes changed, and the Trainer writing its PNG files."""
import os
import struct
import zlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import render_cases as RC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = RC.all_cases()
SENTINEL, GUARD = 0xA5, 256


def _by_name(start, thickness=3):
    return next(c for c in CASES if c["name"].startswith(start) and c["thickness"] == thickness)


def _operands(case):
    """The case on the device: (video, boxes, labels, keywords of ops.render_boxes).  A `gap` puts NaN (f32) or 255
    between the samples' clips, which the kernel must step over."""
    video = torch.from_numpy(case["video"])
    B, L = video.shape[:2]
    n = video[0].numel()
    flat = torch.full((B, n + case["gap"]), float("nan") if video.dtype == torch.float32 else 255, dtype=video.dtype)
    flat[:, :n] = video.reshape(B, n)
    dev = flat.to(DEV)
    video = dev.as_strided(tuple(video.shape), (n + case["gap"],) + tuple(video[0].stride()))
    assert case["gap"] == 0 or not video.is_contiguous()
    kw = dict(mean=torch.from_numpy(RC.MEAN).to(DEV), std=torch.from_numpy(RC.STD).to(DEV),
              palette=torch.from_numpy(RC.PALETTE).to(DEV), thickness=case["thickness"],
              frame_idx=None if case["frame_idx"] is None else torch.tensor(case["frame_idx"], dtype=torch.int32, device=DEV))
    return video, torch.from_numpy(case["boxes"]).to(DEV), torch.from_numpy(case["labels"]).to(DEV), kw


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_kernel_equals_the_restatement(case):
    from future_od.native import ops
    video, boxes, labels, kw = _operands(case)
    want = RC.expected(case)
    n = want.size
    for offset in (0, 1):               # 1: no output row is dword-aligned -- the byte stores
        buf = torch.full((offset + n + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
        out = buf[offset:offset + n].view(want.shape)
        assert ops.render_boxes(video, boxes, labels, out=out, **kw) is out
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert np.array_equal(host[offset:offset + n].reshape(want.shape), want), (case["name"], offset)
        assert (host[:offset] == SENTINEL).all() and (host[offset + n:] == SENTINEL).all()
    fresh = ops.render_boxes(video, boxes, labels, **kw)
    assert fresh.dtype == torch.uint8 and fresh.is_contiguous() and np.array_equal(fresh.cpu().numpy(), want)


def test_render_on_a_device_clip_is_the_kernel_and_equals_the_cpu_form():
    from future_od.utils.visualization import render
    for case in (_by_name("two samples"), _by_name("uint8 source"), _by_name("pixels"), _by_name("labels -1 and P", 1)):
        video, boxes, labels = (torch.from_numpy(case[k]) for k in ("video", "boxes", "labels"))
        idx = None if case["frame_idx"] is None else torch.tensor(case["frame_idx"])           # i64, on the host
        got = render(video.to(DEV), boxes.to(DEV), labels.long().to(DEV), idx, case["thickness"])
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), RC.expected(case)), case["name"]
        assert torch.equal(got.cpu(), render(video, boxes, labels, idx, case["thickness"]))


def test_wrapper_checks_its_operands():
    from future_od.native import lib as L
    from future_od.native import ops
    video, boxes, labels, kw = _operands(_by_name("interior"))
    for bad in (lambda: ops.render_boxes(video, boxes.double(), labels, **kw),
                lambda: ops.render_boxes(video, boxes, labels.long(), **kw),
                lambda: ops.render_boxes(video, boxes[:, :, :3].contiguous(), labels, **kw),
                lambda: ops.render_boxes(video, boxes, labels[:, :0], **kw),
                lambda: ops.render_boxes(video, boxes.cpu(), labels, **kw),
                lambda: ops.render_boxes(video, boxes, labels, **{**kw, "mean": None}),
                lambda: ops.render_boxes(video, boxes, labels, **{**kw, "palette": kw["palette"].float()}),
                lambda: ops.render_boxes(video, boxes, labels, **{**kw, "frame_idx": torch.zeros(2, dtype=torch.int32, device=DEV)}),
                lambda: ops.render_boxes(video, boxes, labels, **{**kw, "thickness": 0}),
                lambda: ops.render_boxes(video, boxes, labels, **{**kw, "thickness": 9}),
                lambda: ops.render_boxes(video[..., ::2], boxes, labels, **kw),
                lambda: ops.render_boxes(video.bfloat16(), boxes, labels, **kw),
                lambda: ops.render_boxes(video[:, :, :2], boxes, labels, **kw),
                lambda: ops.render_boxes(video, boxes, labels, out=torch.empty(1, 23, 17, 3, dtype=torch.uint8, device=DEV), **kw)):
        with pytest.raises(L.FodError, match="render_boxes"):
            bad()


def test_out_is_reused():
    from future_od.native import ops
    a, b = _by_name("interior"), _by_name("reversed")
    va, ba, la, kw = _operands(a)
    vb, bb, lb, _ = _operands(b)
    out = torch.empty(RC.expected(a).shape, dtype=torch.uint8, device=DEV)
    ops.render_boxes(va, ba, la, out=out, **kw)
    first = out.cpu().numpy()
    ops.render_boxes(vb, bb, lb, out=out, **kw)
    assert np.array_equal(first, RC.expected(a)) and np.array_equal(out.cpu().numpy(), RC.expected(b))


def test_on_a_side_stream():
    from future_od.native import ops
    case = _by_name("70 boxes")
    video, boxes, labels, kw = _operands(case)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = ops.render_boxes(video, boxes, labels, **kw)
    side.synchronize()
    assert np.array_equal(out.cpu().numpy(), RC.expected(case))


def test_render_detections():
    from future_od.utils.visualization import render_detections
    case = _by_name("uint8 source")                       # B = 2, six boxes each
    det = {"scores": torch.tensor([[0.9, 0.8, 0.5, 0.49, 0.3, 0.0], [0.95, 0.6, 0.55, 0.0, 0.0, 0.0]]),
           "labels": torch.from_numpy(case["labels"]).clone(), "boxes": torch.from_numpy(case["boxes"]),
           "count": torch.tensor([5, 2], dtype=torch.int32)}
    shown = dict(case, labels=case["labels"].copy(), frame_idx=[1, 0])
    shown["labels"][0, 3:] = -1                           # below min_score
    shown["labels"][1, 2:] = -1                           # slot >= count, whatever its score
    want = RC.expected(shown)
    idx = torch.tensor([1, 0])
    video = torch.from_numpy(case["video"])
    got = render_detections(video.to(DEV), {k: v.to(DEV) for k, v in det.items()}, frame_idx=idx)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(render_detections(video, det, frame_idx=idx).numpy(), want)
    lower = dict(shown, labels=case["labels"].copy())
    lower["labels"][0, 5:], lower["labels"][1, 2:] = -1, -1
    got = render_detections(video.to(DEV), {k: v.to(DEV) for k, v in det.items()}, min_score=0.25, frame_idx=idx)
    assert np.array_equal(got.cpu().numpy(), RC.expected(lower))


def test_a_captured_launch_reads_its_boxes_at_replay():
    from future_od.native import ops
    first, second = _by_name("overlapping"), _by_name("reversed")
    video, boxes, labels, kw = _operands(first)
    boxes, labels = boxes[:, :3].contiguous(), labels[:, :3].contiguous()          # both cases at three boxes
    first = dict(first, boxes=first["boxes"][:, :3], labels=first["labels"][:, :3])
    out = torch.zeros(RC.expected(first).shape, dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.render_boxes(video, boxes, labels, out=out, **kw)                      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.render_boxes(video, boxes, labels, out=out, **kw)
    out.zero_()
    graph.replay()
    assert np.array_equal(out.cpu().numpy(), RC.expected(first))
    boxes.copy_(torch.from_numpy(second["boxes"]))
    labels.copy_(torch.from_numpy(second["labels"]))
    graph.replay()
    assert np.array_equal(out.cpu().numpy(), RC.expected(dict(second, video=first["video"])))


# ---- the Trainer ---------------------------------------------------------------------------------------------------------
class _Loader(list):
    batch_size = 2


def _decode(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    w, h = struct.unpack(">II", data[16:24])
    n = struct.unpack(">I", data[33:37])[0]
    assert data[37:41] == b"IDAT"
    raw = np.frombuffer(zlib.decompress(data[41:41 + n]), dtype=np.uint8).reshape(h, 1 + 3 * w)
    return raw[:, 1:].reshape(h, w, 3)


def _train_one_epoch(path, batches, epochs, iterations):
    from future_od.models.st_detr import SpatioTemporalDETRArgs
    from future_od.native import functional as Fn
    from future_od.trainer import Trainer
    from runs._helper import get_lr_func, setup_optimizer
    from runs._model import build_model
    torch.manual_seed(0)
    Fn.manual_seed(0)
    args = SimpleNamespace(device=DEV, distributed=False, compute_dtype="bf16", backbone="resnet18")
    detr = SpatioTemporalDETRArgs(num_classes=8, num_queries=32, lr_backbone=1e-4, enc_layers=1, dec_layers=2,
                                  pretrained_backbone=False)
    model = build_model(args, detr)
    sched, opt = setup_optimizer(detr, model, get_lr_func(4))
    tr = Trainer(model, opt, sched, _Loader(batches), {"val": _Loader(batches[:1])}, str(path), str(path), "t", DEV,
                 print_interval=3, visualization_epochs=epochs, visualization_iterations=iterations, category_dict={},
                 is_master=True, max_norm=detr.max_norm)
    tr.train(1)
    torch.cuda.synchronize()
    assert tr._graphed not in (None, False) and tr._graphed.replays == len(batches)
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def test_trainer_writes_the_pictures_and_trains_the_same(tmp_path):
    from future_od.datasets.synthetic import make_batch
    from future_od.native import ops
    from future_od.utils.visualization import render
    prev = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        batches = [make_batch(2, 3, 96, 128, seed=s, max_boxes=5) for s in (1, 2, 3)]
        seen, blind = tmp_path / "seen", tmp_path / "blind"
        with_pictures = _train_one_epoch(seen, batches, [1], [0])
        without = _train_one_epoch(blind, batches, [], [])
    finally:
        ops.set_deterministic(prev)
    names = {f"{mode}_b{b}_{kind}.png" for mode in ("train", "val") for b in (0, 1) for kind in ("anno", "pred")}
    assert set(os.listdir(seen)) == names and not os.path.exists(blind)
    first = batches[0]
    labels = first["classes"].masked_fill(first["active"] == 0, -1)
    want = render(first["video"].to(DEV), first["boxes"].to(DEV), labels.to(DEV), first["annotated_frame_idx"]).cpu().numpy()
    assert not np.array_equal(want, render(first["video"], first["boxes"], labels * 0 - 1, first["annotated_frame_idx"]).numpy())
    for mode in ("train", "val"):
        for b in (0, 1):
            anno, pred = _decode(seen / f"{mode}_b{b}_anno.png"), _decode(seen / f"{mode}_b{b}_pred.png")
            assert anno.shape == pred.shape == (96, 128, 3)
            assert np.array_equal(anno, want[b]), (mode, b)
    assert set(with_pictures) == set(without)
    bad = [k for k in without if not torch.equal(with_pictures[k], without[k])]
    assert not bad, bad[:8]
