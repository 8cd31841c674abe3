"""fod_render_labels on the device: every case of tests/label_cases.py against the numpy restatement byte for byte on
pictures pre-filled with random bytes (aligned and unaligned, a guard band around them), the wrapper's refusals, `render`
and `render_detections` with captions against their CPU forms, a side stream, a captured launch replayed after its
detections changed, and the Trainer writing captioned PNG files."""
import os
import struct
import zlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import label_cases as LC
from future_od.utils import visualization as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = LC.all_cases(V.FONT_5X7.numpy())
SENTINEL, GUARD = 0xA5, 256


def _by_name(start):
    return next(c for c in CASES if c["name"].startswith(start))


def _dev(array):
    return None if array is None else torch.from_numpy(array).to(DEV)


def captions_of(case):
    """(Captions, palette as `render` takes it) of a case."""
    t = lambda array: None if array is None else torch.from_numpy(array)
    captions = V.Captions(names=t(case["names"]), ident=t(case["idents"]), scores=t(case["scores"]), scale=case["scale"],
                          font=t(case["font"]), font_first=case["font_first"], font_width=case["font_width"])
    palette = V.COLOURS if case["palette"] is LC.PALETTE else t(case["palette"]).float() / 255          # 0 and 255 only
    return captions, palette


def clip_of(case):
    return torch.from_numpy(LC.clip_of(case))


def _operands(case):
    """(boxes, labels, keywords of ops.render_labels) of the case on the device."""
    kw = dict(idents=_dev(case["idents"]), scores=_dev(case["scores"]), names=_dev(case["names"]),
              palette=_dev(case["palette"]), font=_dev(case["font"]), font_first=case["font_first"],
              font_width=case["font_width"], scale=case["scale"], thickness=case["thickness"])
    return _dev(case["boxes"]), _dev(case["labels"]), kw


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_kernel_equals_the_restatement(case):
    from future_od.native import ops
    boxes, labels, kw = _operands(case)
    want = LC.expected(case)
    n = want.size
    for offset in (0, 1):               # 1: no row of the pictures is dword-aligned -- the byte stores
        buf = torch.full((GUARD + offset + n + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
        pictures = buf[GUARD + offset:GUARD + offset + n].view(want.shape)
        pictures.copy_(torch.from_numpy(case["picture"]))
        assert ops.render_labels(pictures, boxes, labels, **kw) is pictures
        host = buf.cpu()
        assert np.array_equal(host[GUARD + offset:GUARD + offset + n].view(want.shape).numpy(), want), (case["name"], offset)
        assert bool((host[:GUARD + offset] == SENTINEL).all()) and bool((host[GUARD + offset + n:] == SENTINEL).all())


def test_wrapper_refuses_bad_operands_and_launches_nothing():
    from future_od.native import lib as L
    from future_od.native import ops
    case = _by_name("mixed 24x40 s1 t3")
    boxes, labels, kw = _operands(case)
    start = _dev(case["picture"])
    pictures = start.clone()
    font = kw["font"]
    for bad in (lambda: ops.render_labels(pictures.cpu(), boxes, labels, **kw),
                lambda: ops.render_labels(pictures.float(), boxes, labels, **kw),
                lambda: ops.render_labels(pictures[:, :, ::2], boxes, labels, **kw),
                lambda: ops.render_labels(pictures[..., :2], boxes, labels, **kw),
                lambda: ops.render_labels(pictures, boxes.double(), labels, **kw),
                lambda: ops.render_labels(pictures, boxes, labels.long(), **kw),
                lambda: ops.render_labels(pictures, boxes[:, :, :3].contiguous(), labels, **kw),
                lambda: ops.render_labels(pictures, boxes, labels[:, :5].contiguous(), **kw),
                lambda: ops.render_labels(pictures, boxes.cpu(), labels, **kw),
                lambda: ops.render_labels(pictures, boxes, labels, **{**kw, "idents": kw["idents"].long()}),
                lambda: ops.render_labels(pictures, boxes, labels, **{**kw, "idents": kw["idents"][:, :5].contiguous()}),
                lambda: ops.render_labels(pictures, boxes, labels, **{**kw, "scores": kw["scores"].double()}),
                lambda: ops.render_labels(pictures, boxes, labels, **{**kw, "scores": kw["scores"].cpu()}),
                lambda: ops.render_labels(pictures, boxes, labels, **{**kw, "names": kw["names"].int()}),
                lambda: ops.render_labels(pictures, boxes, labels, **{**kw, "names": kw["names"][0]}),
                lambda: ops.render_labels(pictures, boxes, labels, **{**kw, "names": torch.zeros(4, 33, dtype=torch.uint8, device=DEV)}),
                lambda: ops.render_labels(pictures, boxes, labels, **{**kw, "palette": kw["palette"].float()}),
                lambda: ops.render_labels(pictures, boxes, labels, **{**kw, "palette": kw["palette"][:, :2].contiguous()}),
                lambda: ops.render_labels(pictures, boxes, labels, **{**kw, "font": font.float()}),
                lambda: ops.render_labels(pictures, boxes, labels, **{**kw, "font": font[0]}),
                lambda: ops.render_labels(pictures, boxes, labels, **{**kw, "font": torch.zeros(4, 17, dtype=torch.uint8, device=DEV)}),
                lambda: ops.render_labels(pictures, boxes, labels, **{**kw, "font_first": 200}),
                lambda: ops.render_labels(pictures, boxes, labels, **{**kw, "font_first": -1}),
                lambda: ops.render_labels(pictures, boxes, labels, **{**kw, "font_width": 0}),
                lambda: ops.render_labels(pictures, boxes, labels, **{**kw, "font_width": 9}),
                lambda: ops.render_labels(pictures, boxes, labels, **{**kw, "scale": 0}),
                lambda: ops.render_labels(pictures, boxes, labels, **{**kw, "scale": 9}),
                lambda: ops.render_labels(pictures, boxes, labels, **{**kw, "thickness": 0}),
                lambda: ops.render_labels(pictures, boxes, labels, **{**kw, "thickness": 13}),
                lambda: ops.render_labels(pictures, torch.zeros(1, 1025, 4, device=DEV),
                                          torch.zeros(1, 1025, dtype=torch.int32, device=DEV),
                                          **{**kw, "idents": None, "scores": None})):
        with pytest.raises(L.FodError, match="render_labels"):
            bad()
    assert torch.equal(pictures, start)                    # nothing was launched


def test_render_with_captions_on_a_device_clip_equals_the_restatement_and_the_cpu_form():
    for start in ("mixed 40x300 s2 t3", "mixed 18x262 s1 t1", "font 8x16 random 24x40", "two samples 40x300",
                  "a short name table", "skipped labels", "no operand at all"):
        case = _by_name(start)
        captions, palette = captions_of(case)
        video, boxes, labels = clip_of(case), torch.from_numpy(case["boxes"]), torch.from_numpy(case["labels"])
        got = V.render(video.to(DEV), boxes.to(DEV), labels.long().to(DEV), None, case["thickness"], palette, captions=captions)
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), LC.expected_over_outlines(case)), case["name"]
        assert torch.equal(got.cpu(), V.render(video, boxes, labels, None, case["thickness"], palette, captions=captions))
        plain = V.render(video.to(DEV), boxes.to(DEV), labels.to(DEV), None, case["thickness"], palette)
        assert torch.equal(V.render(video.to(DEV), boxes.to(DEV), labels.to(DEV), None, case["thickness"], palette,
                                    captions=None), plain)


def _detections(case):
    """What predict() returns, made of a two-sample case: (clip, det) on the host."""
    labels = torch.from_numpy(case["labels"]).clamp(0, LC.P - 1)
    B, K = labels.shape
    det = {"scores": torch.linspace(0.05, 0.95, B * K).view(B, K).contiguous(), "labels": labels,
           "boxes": torch.from_numpy(case["boxes"]).clone(), "query": torch.from_numpy(case["idents"]).clamp_min(0),
           "count": torch.tensor([K, K - 3], dtype=torch.int32)}
    return clip_of(case), det


def test_render_detections_with_captions_equals_its_cpu_form():
    video, det = _detections(_by_name("two samples 40x300"))
    on = {k: v.to(DEV) for k, v in det.items()}
    for ident in ("slot", "query", None):
        for scores in (True, False):
            captions = V.Captions(names=LC.NAME_LIST, ident=ident, scores=scores)
            got = V.render_detections(video.to(DEV), on, frame_idx=torch.tensor([0, -1]), captions=captions)
            want = V.render_detections(video, det, frame_idx=torch.tensor([0, -1]), captions=captions)
            assert got.is_cuda and torch.equal(got.cpu(), want), (ident, scores)
    assert not torch.equal(want, V.render_detections(video, det))


def test_on_a_side_stream():
    from future_od.native import ops
    case = _by_name("257 labels 40x300")
    boxes, labels, kw = _operands(case)
    pictures = _dev(case["picture"])
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.render_labels(pictures, boxes, labels, **kw)
    side.synchronize()
    assert np.array_equal(pictures.cpu().numpy(), LC.expected(case))


def test_a_captured_launch_reads_its_detections_at_replay():
    first, second = _by_name("two samples 40x300"), _by_name("two samples 18x262")
    video, det = _detections(first)
    _, other = _detections(second)                         # other boxes, labels, queries and scores of the same extent
    other["boxes"] = other["boxes"] * torch.tensor([300 / 262, 40 / 18, 300 / 262, 40 / 18])
    other["count"] = torch.tensor([4, 9], dtype=torch.int32)
    video_on, on = video.to(DEV), {k: v.to(DEV) for k, v in det.items()}
    captions = V.Captions(names=LC.NAME_LIST, ident="query", scores=True)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        V.render_detections(video_on, on, captions=captions)                       # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = V.render_detections(video_on, on, captions=captions)
    graph.replay()
    assert torch.equal(out.cpu(), V.render_detections(video, det, captions=captions))
    for k, v in other.items():
        on[k].copy_(v)
    graph.replay()
    want = V.render_detections(video, other, captions=captions)
    assert torch.equal(out.cpu(), want) and not torch.equal(want, V.render_detections(video, det, captions=captions))
    assert torch.equal(out, V.render_detections(video_on, on, captions=captions))          # eager, on the device


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


CATEGORIES = {0: "car", 1: "truck", 2: "ConstructionVehicle", 3: "bus", 4: "pedestrian", 5: "cone", 6: "barrier", 7: "bike"}


def _train_one_epoch(path, batches, captions):
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
                 print_interval=3, visualization_epochs=[1], visualization_iterations=[0], category_dict=CATEGORIES,
                 is_master=True, max_norm=detr.max_norm)
    if captions is not None:
        assert tr.set_captions(captions) is tr
    seen = {}
    plain = tr.visualize_batch

    def spy(data, model_output, mode, log_to_wandb, prefix=""):
        seen[mode] = ({k: v.detach().clone() if isinstance(v, torch.Tensor) else v for k, v in data.items()},
                      {k: model_output[k].detach().clone() for k in ("class_scores", "boxes")})
        return plain(data, model_output, mode, log_to_wandb, prefix)
    tr.visualize_batch = spy
    tr.train(1)
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in model.state_dict().items()}, seen


def test_trainer_writes_captioned_pictures_and_trains_the_same(tmp_path):
    from future_od.datasets.synthetic import make_batch
    from future_od.native import ops
    prev = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        batches = [make_batch(2, 3, 96, 128, seed=s, max_boxes=5) for s in (1, 2)]
        on, off, never = tmp_path / "on", tmp_path / "off", tmp_path / "never"
        with_captions, seen = _train_one_epoch(on, batches, True)
        switched_off, _ = _train_one_epoch(off, batches, False)
        untouched, _ = _train_one_epoch(never, batches, None)
    finally:
        ops.set_deterministic(prev)
    files = sorted(os.listdir(never))
    assert len(files) == 8 and sorted(os.listdir(on)) == files == sorted(os.listdir(off))
    for f in files:                                        # off: byte-identical files
        assert open(off / f, "rb").read() == open(never / f, "rb").read(), f
    # on: the pictures are the CPU form's, from the batch and the model output the Trainer was handed
    for mode in ("train", "val"):
        data, output = seen[mode]
        host = lambda t: t.detach().float().cpu() if t.is_floating_point() else t.detach().cpu()
        scores, boxes = host(output["class_scores"][:, :, -1]), host(output["boxes"][:, :, -1])
        B, L_out, M, _ = scores.shape
        frame = host(data["annotated_frame_idx"])
        L_in = data["video"].shape[1]
        at = torch.where(frame < 0, frame + L_in, frame).clamp(0, L_in - 1) if L_out == L_in else torch.zeros(B, dtype=torch.int64)
        scores, boxes = scores[torch.arange(B), at], boxes[torch.arange(B), at]
        best, classes = scores.max(dim=2)
        classes = classes.masked_fill(best < 0.5, -1)
        anno_classes = host(data["classes"]).masked_fill(host(data["active"]) == 0, -1)
        anno_boxes = host(data["boxes"])
        A = anno_classes.shape[1]
        video = host(data["video"])
        anno = V.render(video, anno_boxes, anno_classes, frame, captions=V.Captions(names=CATEGORIES))
        idents = torch.cat([torch.full((B, A), -1, dtype=torch.int32), torch.arange(M, dtype=torch.int32)[None].expand(B, M)], 1)
        shown = torch.cat([torch.full((B, A), float("nan")), best], 1)
        pred = V.render(video, torch.cat([anno_boxes, boxes], 1), torch.cat([anno_classes, classes], 1), frame,
                        captions=V.Captions(names=CATEGORIES, ident=idents, scores=shown))
        assert not torch.equal(anno, V.render(video, anno_boxes, anno_classes, frame))      # there is text in it
        for b in range(B):
            assert np.array_equal(_decode(on / f"{mode}_b{b}_anno.png"), anno[b].numpy()), (mode, b)
            assert np.array_equal(_decode(on / f"{mode}_b{b}_pred.png"), pred[b].numpy()), (mode, b)
    for other in (switched_off, untouched):                # the epoch's parameters: bit-equal with and without captions
        assert set(with_captions) == set(other)
        bad = [k for k in other if not torch.equal(with_captions[k], other[k])]
        assert not bad, bad[:8]
