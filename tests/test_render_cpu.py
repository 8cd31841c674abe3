"""The box renderer, the parts that need no GPU: the entry point as the binding reads it from include/fod_ext.h and its
argument checks, the CPU form (visualization.draw_boxes / render) against the numpy restatement of tests/render_cases.py
bit for bit and against outputs recorded from the reference's own draw_boxes, the PNG writer, the W&B box dictionaries,
and the Trainer's surface."""
import inspect
import os
import re
import struct
import zlib

import numpy as np
import pytest
import torch

import render_cases as RC
from future_od.native import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, LONG = "pointer", "int", "long"
ENTRY = "fod_render_boxes"
CASES = RC.all_cases()


# ---- ABI and binding ---------------------------------------------------------------------------------------------------
def test_prototype_is_read_from_the_second_header():
    assert abi.EXT_PROTOTYPES[ENTRY] == (I, [P, I, P, I, I, I, I, LONG, LONG, P, P, P, P, P, I, P, I, I, P])
    assert ENTRY not in abi.PROTOTYPES and ENTRY not in open(abi.HEADER_PATH).read()
    from future_od.native import lib as L
    assert ENTRY in L.EXT_SIGNATURES and ENTRY in L._ENTRY and ENTRY not in L.SIGNATURES and ENTRY not in L.FAST
    fn = getattr(L.LIB, ENTRY)
    assert fn.restype is abi.CTYPE[I] and list(fn.argtypes) == [abi.CTYPE[k] for k in abi.EXT_PROTOTYPES[ENTRY][1]]


def test_abi_version_moved_with_the_entry_point():
    from future_od.native import lib as L
    hdr = open(os.path.join(ROOT, "include", "fod.h")).read()
    assert int(re.search(r"#define FOD_ABI_VERSION (\d+)", hdr).group(1)) == L.ABI_VERSION == L.LIB.fod_abi_version() >= 13


def _entry(src=1, u8=0, dst=1, B=1, L=1, H=16, W=16, sb=768, sl=768, idx=None, mean=1, std=1, boxes=1, labels=1, N=1,
           palette=1, P=125, t=3):
    """The non-null 'pointers' are the address 1: a launch would fault, so a clean non-zero return is the check itself."""
    from future_od.native import lib
    rc = getattr(lib.LIB, ENTRY)(src, u8, dst, B, L, H, W, sb, sl, idx, mean, std, boxes, labels, N, palette, P, t, None)
    return rc, lib.last_error()


@pytest.mark.parametrize("kw, text", [
    (dict(t=0), "thickness"), (dict(t=-2), "thickness"),
    (dict(H=5), "thickness 3"), (dict(W=5), "thickness 3"), (dict(H=1, W=1, sb=3, sl=3, t=1), "thickness 1"),
    (dict(N=1025), "1025 boxes"), (dict(N=-1), "-1 boxes"),
    (dict(P=0), "palette"), (dict(P=-3), "palette"),
    (dict(mean=None), "mean and std"), (dict(std=None), "mean and std"),
    (dict(src=None), "null"), (dict(dst=None), "null"), (dict(boxes=None), "null"), (dict(labels=None), "null"),
    (dict(palette=None), "null"), (dict(sl=767), "strides"), (dict(sb=100), "strides"), (dict(B=0), "extent"),
    (dict(L=0), "extent"), (dict(B=65536), "extent"),
])
def test_arguments_are_refused_before_any_launch(kw, text):
    from future_od.native import lib as L
    rc, err = _entry(**kw)
    assert rc == L.ERR_ARG and "render_boxes" in err and text in err, (kw, rc, err)


def test_refusals_with_null_pointers_and_through_call():
    """Every refusal of the entry's list also with ALL pointers null: the argument is named, nothing is launched."""
    from future_od.native import lib as L
    null = dict(src=None, dst=None, mean=None, std=None, boxes=None, labels=None, palette=None)
    for kw, text in ((dict(t=0), "thickness"), (dict(H=4), "thickness 3"), (dict(W=5), "thickness 3"),
                     (dict(N=1025), "1025 boxes"), (dict(N=-1), "-1 boxes"), (dict(P=0), "palette"), ({}, "mean and std")):
        rc, err = _entry(**{**null, **kw})
        assert rc == L.ERR_ARG and text in err, (kw, err)
    with pytest.raises(L.FodError, match="render_boxes.*thickness"):
        L.call(ENTRY, None, 0, None, 1, 1, 16, 16, 768, 768, None, None, None, None, None, 0, None, 1, 0, None)


def test_wrapper_has_no_cpu_fallback():
    from future_od.native import lib as L
    from future_od.native import ops
    video = torch.zeros(1, 1, 3, 8, 8)
    kw = dict(mean=torch.zeros(3), std=torch.ones(3), palette=torch.zeros(4, 3, dtype=torch.uint8))
    with pytest.raises(L.FodError, match="render_boxes.*no CPU fallback"):
        ops.render_boxes(video, torch.zeros(1, 0, 4), torch.zeros(1, 0, dtype=torch.int32), **kw)
    with pytest.raises(L.FodError, match="render_boxes.*no CPU fallback"):
        ops.render_boxes(video.to(torch.uint8), torch.zeros(1, 0, 4), torch.zeros(1, 0, dtype=torch.int32), **kw)


# ---- the CPU form ------------------------------------------------------------------------------------------------------
def test_colours():
    from future_od.utils.visualization import COLOURS, to_bytes
    assert COLOURS.dtype == torch.float32 and tuple(COLOURS.shape) == (125, 3)
    assert COLOURS[1].tolist() == [0.25, 0, 0] and COLOURS[5].tolist() == [0, 0.25, 0] and COLOURS[25].tolist() == [0, 0, 0.25]
    assert COLOURS[124].tolist() == [1, 1, 1] and COLOURS[0].tolist() == [0, 0, 0]
    lv = (0, .25, .5, .75, 1)
    for i in (7, 38, 93, 111):
        a, b, c = i // 25, i // 5 % 5, i % 5
        assert COLOURS[i].tolist() == [lv[c], lv[b], lv[a]]
    assert np.array_equal(to_bytes(COLOURS).numpy(), RC.PALETTE)          # 63, 127, 191, 255: truncated


def test_the_restatement_paints_what_it_says():
    """The restatement against pixels worked out by hand: a 3..9 x 2..6 box, thickness 1, on an 8 x 12 uint8 frame."""
    frame = np.zeros((3, 8, 12), dtype=np.uint8)
    img = RC.paint(RC.background(frame), np.array([[3, 2, 9, 6]], dtype=np.float32), [124], 1)
    want = np.zeros((8, 12), dtype=bool)
    want[1:6, 2] = True       # left   [Tp-1, Bt) x [Lf-1, Lf)
    want[6, 2:9] = True       # bottom [Bt, Bt+1) x [Lf-1, Rt)
    want[2:7, 9] = True       # right  [Tp, Bt+1) x [Rt, Rt+1)
    want[1, 3:10] = True      # top    [Tp-1, Tp) x [Lf, Rt+1)
    assert np.array_equal(img[..., 0] == 255, want) and np.array_equal(img[..., 2] == 255, want)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_cpu_render_equals_the_restatement(case):
    from future_od.utils.visualization import render
    idx = None if case["frame_idx"] is None else torch.tensor(case["frame_idx"])
    labels = torch.from_numpy(case["labels"])
    for lab in (labels, labels.long()):
        got = render(torch.from_numpy(case["video"]), torch.from_numpy(case["boxes"]), lab, idx, case["thickness"])
        assert got.dtype == torch.uint8 and got.is_contiguous()
        assert np.array_equal(got.numpy(), RC.expected(case))


def test_draw_boxes_is_in_place_and_checks_the_thickness():
    from future_od.utils.visualization import COLOURS, draw_boxes
    image = torch.zeros(3, 12, 12)
    assert draw_boxes(image, torch.tensor([[3.0, 3.0, 8.0, 8.0]]), COLOURS[[124]], 2) is image and image.sum() > 0
    for t, size in ((0, 12), (3, 5)):
        with pytest.raises(ValueError, match="thickness"):
            draw_boxes(torch.zeros(3, size, size), torch.zeros(1, 4), COLOURS[:1], t)


def test_cpu_form_equals_the_reference_fixture(golden):
    """tests/golden/draw_boxes_ref.npz: inputs and float outputs of the reference's own draw_boxes
    (tests/golden/make_render_golden.py), drawable cases only."""
    from future_od.utils.visualization import draw_boxes
    g = golden("draw_boxes_ref")
    names, meta = [str(n) for n in g["names"]], g["meta"]
    assert len(names) == len(meta) >= 40 and set(meta[:, 2].tolist()) == {1, 3}
    for name, (h, w, t, n, slot), boxes, colours in zip(names, meta.tolist(), g["boxes"], g["colours"]):
        image = torch.from_numpy(g[f"image_{h}x{w}"].copy())
        got = draw_boxes(image, torch.from_numpy(boxes[:n]), torch.from_numpy(colours[:n]), t)
        assert np.array_equal(got.numpy(), g[f"out_{h}x{w}"][slot]), name


# ---- PNG ---------------------------------------------------------------------------------------------------------------
def _read_png(path):
    """(width, height, uint8 [H, W, 3]) by hand: signature, chunk CRCs, IHDR fields, one IDAT inflated, filter bytes."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF, kind
        chunks.append((kind, body))
        at += 12 + n
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"] and chunks[2][1] == b""
    w, h, depth, colour, compression, filt, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, compression, filt, interlace) == (8, 2, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), dtype=np.uint8).reshape(h, 1 + 3 * w)
    assert not raw[:, 0].any()                                           # filter 0 on every line
    return w, h, raw[:, 1:].reshape(h, w, 3)


def test_write_png_round_trip(tmp_path):
    from future_od.utils.visualization import write_png
    img = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (13, 21, 3), dtype=np.uint8))
    path = str(tmp_path / "new" / "dir" / "a.png")                        # the directory is created
    write_png(img, path)
    w, h, pixels = _read_png(path)
    assert (w, h) == (21, 13) and np.array_equal(pixels, img.numpy())
    write_png(img.numpy(), path)                                          # arrays too, and an existing directory
    assert np.array_equal(_read_png(path)[2], img.numpy())
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        with Image.open(path) as im:
            assert im.mode == "RGB" and im.size == (21, 13) and np.array_equal(np.asarray(im), img.numpy())
    for bad in (img.float(), img[..., :2], img[0]):
        with pytest.raises(ValueError, match="write_png"):
            write_png(bad, path)


def test_visualize_writes_the_rendered_frame(tmp_path, capsys):
    from future_od.utils.visualization import render, visualize
    case = next(c for c in CASES if c["name"].startswith("overlapping") and c["thickness"] == 3)
    image, boxes = torch.from_numpy(case["video"][0, 0]), torch.from_numpy(case["boxes"][0])
    classes = torch.tensor([3, 9, 90, 9])                                  # 9: the background class here
    path = str(tmp_path / "vis" / "val_b0_anno.png")
    got = visualize(image, classes, boxes, path, 9)
    assert capsys.readouterr().out == f"Storing visualization at {path}\n"
    want = render(image[None, None], boxes[[0, 2]][None], classes[[0, 2]][None])[0]
    assert torch.equal(got, want) and np.array_equal(_read_png(path)[2], want.numpy())
    scores = torch.zeros(4, 12)                                           # scores: best class, background below 0.5
    scores[0, 3], scores[1, 5], scores[2, 90 % 12], scores[3, 7] = 0.9, 0.49, 0.5, 0.2
    got = visualize(image, scores, boxes, path, 12)
    want = render(image[None, None], boxes[[0, 2]][None], torch.tensor([[3, 90 % 12]]))[0]
    assert torch.equal(got, want)
    assert torch.equal(visualize(image, None, None, path, 12), render(image[None, None], boxes[:0][None], classes[:0][None])[0])


# ---- W&B ---------------------------------------------------------------------------------------------------------------
def test_wandb_box_data():
    from future_od.utils.visualization import visualize_wandb, wandb_box_data
    names = {0: "car", 1: "truck", 2: "bus"}
    scores = torch.tensor([[0.05, 0.8, 0.1], [0.09, 0.05, 0.02], [0.3, 0.2, 0.6]])
    pred = torch.tensor([[1.4, 2.5, 10.6, 20.5], [0.0, 0.0, 5.0, 5.0], [3.5, 4.5, 7.49, 8.51]])
    anno_cls, anno = torch.tensor([2, 3, 0]), torch.tensor([[1.0, 2.0, 3.0, 4.0], [9.0, 9.0, 9.0, 9.0], [5.6, 6.4, 7.5, 8.5]])
    ignore = torch.tensor([[0.0, 0.0, 2.2, 2.7]])
    got = wandb_box_data(3, names, scores, pred, anno_cls, anno, ignore)
    assert got == {
        "predictions": {"box_data": [
            {"position": {"minX": 1, "maxX": 11, "minY": 2, "maxY": 20}, "domain": "pixel", "class_id": 1,
             "scores": {"score": pytest.approx(0.8)}, "box_caption": "0 truck"},
            {"position": {"minX": 4, "maxX": 7, "minY": 4, "maxY": 9}, "domain": "pixel", "class_id": 2,
             "scores": {"score": pytest.approx(0.6)}, "box_caption": "2 bus"}], "class_labels": names},
        "ground_truth": {"box_data": [
            {"position": {"minX": 1, "maxX": 3, "minY": 2, "maxY": 4}, "domain": "pixel", "class_id": 2},
            {"position": {"minX": 6, "maxX": 8, "minY": 6, "maxY": 8}, "domain": "pixel", "class_id": 0}],
            "class_labels": names},
        "ignore_regions": {"box_data": [{"position": {"minX": 0, "maxX": 2, "minY": 0, "maxY": 3}, "domain": "pixel",
                                         "class_id": 0}], "class_labels": {0: "Ignore"}}}
    for data in got.values():
        for box in data["box_data"]:
            assert all(type(v) is int for v in box["position"].values()) and type(box["class_id"]) is int
    assert wandb_box_data(3, names) == {} and set(wandb_box_data(3, names, anno_classes=anno_cls, anno_boxes=anno)) == {"ground_truth"}
    try:
        import wandb  # noqa: F401
    except ImportError:
        with pytest.raises(RuntimeError, match="wandb"):
            visualize_wandb(torch.zeros(3, 4, 4), 3, names)


# ---- Trainer -----------------------------------------------------------------------------------------------------------
def test_trainer_surface():
    from future_od.trainer import Trainer
    assert list(inspect.signature(Trainer.visualize_batch).parameters) == ["self", "data", "model_output", "mode",
                                                                           "log_to_wandb", "prefix"]
    assert inspect.signature(Trainer.visualize_batch).parameters["prefix"].default == ""
    assert list(inspect.signature(Trainer.__init__).parameters) == [
        "self", "model", "optimizer", "lr_sched", "train_loader", "val_loaders", "checkpoint_path", "visualization_path",
        "save_name", "device", "print_interval", "visualization_epochs", "visualization_iterations", "category_dict",
        "checkpoint_epochs", "gradient_clip_value", "distributed", "is_master", "wandb_config", "max_norm", "ema"]


@pytest.mark.parametrize("queries", [12, 900])
def test_visualize_batch_on_host_tensors(tmp_path, queries):
    """The method's bookkeeping without a GPU (CPU tensors go through the CPU form): file names, the annotated frame, active
    annotations only, predictions from 0.5 on top of them, and -- with more queries than the renderer's 1024 boxes leave
    room for beside the 256 annotation slots -- the best-scoring ones."""
    from types import SimpleNamespace
    from future_od.datasets.synthetic import make_batch
    from future_od.trainer import Trainer
    from future_od.utils.visualization import render
    data = make_batch(2, 3, 24, 40, seed=1, max_boxes=5)
    data["annotated_frame_idx"] = torch.tensor([-1, 1])
    g = torch.Generator().manual_seed(queries)
    scores = torch.rand(2, 1, 1, queries, 8, generator=g) * 0.53
    boxes = torch.rand(2, 1, 1, queries, 4, generator=g) * 20 + torch.tensor([0.0, 0.0, 12.0, 4.0])
    me = SimpleNamespace(_visualization_path=str(tmp_path / "vis"), _wandb_config=SimpleNamespace(num_images=4),
                         _category_dict={}, _epoch=1)
    Trainer.visualize_batch(me, data, {"class_scores": scores, "boxes": boxes, "moods": None}, "val", False, prefix="x_")
    assert sorted(os.listdir(tmp_path / "vis")) == sorted(f"x_val_b{b}_{k}.png" for b in (0, 1) for k in ("anno", "pred"))
    labels = data["classes"].masked_fill(data["active"] == 0, -1)
    anno = render(data["video"], data["boxes"], labels, data["annotated_frame_idx"])
    best, cls = scores[:, 0, 0].max(dim=2)
    cls = cls.masked_fill(best < 0.5, -1)
    assert 0 < int((cls >= 0).sum()) < cls.numel()
    if queries > 768:
        keep = best.topk(768, dim=1).indices.sort(dim=1).values
        assert int((cls.gather(1, keep) >= 0).sum()) == int((cls >= 0).sum())      # no shown prediction is lost here
        cls, pb = cls.gather(1, keep), boxes[:, 0, 0].gather(1, keep[..., None].expand(-1, -1, 4))
    else:
        pb = boxes[:, 0, 0]
    pred = render(data["video"], torch.cat([data["boxes"], pb], 1), torch.cat([labels, cls], 1), data["annotated_frame_idx"])
    assert not torch.equal(anno, pred)
    for b in (0, 1):
        assert np.array_equal(_read_png(str(tmp_path / "vis" / f"x_val_b{b}_anno.png"))[2], anno[b].numpy())
        assert np.array_equal(_read_png(str(tmp_path / "vis" / f"x_val_b{b}_pred.png"))[2], pred[b].numpy())
