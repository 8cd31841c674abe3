"""Host side of the joint crop / resize augmentation: the transforms' annotation rules against a list-based
restatement, plan() against __call__, the dense-batch form of DeviceJointTransform.host, and the loaders."""
import random
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F


# ---- the rules, restated on Python lists (boxes: lists of [x0, y0, x1, y1], classes: list of ints) ---------------------
def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def ref_crop(boxes, classes, left, top, width, height):
    out_b, out_c = [], []
    for (x0, y0, x1, y1), c in zip(boxes, classes):
        x0, y0, x1, y1 = _f32(x0 - left), _f32(y0 - top), _f32(x1 - left), _f32(y1 - top)
        if x0 <= width and y0 <= height and x1 >= 0 and y1 >= 0:
            out_b.append([min(max(x0, 0.0), width), min(max(y0, 0.0), height), min(max(x1, 0.0), width),
                          min(max(y1, 0.0), height)])
            out_c.append(c)
    return out_b, out_c


def ref_resize(boxes, classes, old_w, old_h, new_w, new_h):
    ws, hs = _f32(new_w / old_w), _f32(new_h / old_h)
    return [[_f32(x0 * ws), _f32(y0 * hs), _f32(x1 * ws), _f32(y1 * hs)] for x0, y0, x1, y1 in boxes], list(classes)


def ref_flip(boxes, classes, w):
    return [[_f32(w - x1), y0, _f32(w - x0), y1] for x0, y0, x1, y1 in boxes], list(classes)


def ref_size_filter(boxes, classes, w, h, min_size):
    keep = [_f32(_f32(_f32(x1 - x0) * _f32(y1 - y0)) / (h * w)) > min_size for x0, y0, x1, y1 in boxes]
    return [b for b, k in zip(boxes, keep) if k], [c for c, k in zip(classes, keep) if k]


H0, W0 = 60, 100
IGNORE = 8          # an ignore-category id rides through like any class


def _case_boxes(left, top, width, height):
    """Boxes placed relative to the crop rectangle (left, top, width, height) of an H0 x W0 frame."""
    r, b = left + width, top + height
    boxes = [
        [left + 5, top + 5, left + 15, top + 12],          # wholly inside
        [left - 6, top + 3, left + 6, top + 9],            # straddles the left edge
        [r - 4, top + 3, r + 7, top + 9],                  # ... the right edge
        [left + 8, top - 5, left + 20, top + 4],           # ... the top edge
        [left + 8, b - 3, left + 20, b + 6],               # ... the bottom edge
        [left - 12, top + 3, left - 2, top + 9],           # wholly outside on the left
        [r + 2, top + 3, r + 9, top + 9],                  # ... right
        [left + 8, top - 9, left + 20, top - 1],           # ... above
        [left + 8, b + 1, left + 20, b + 7],               # ... below
        [left - 7, top + 3, left, top + 9],                # touches the left edge exactly: x1 == 0, kept (inclusive)
        [r, top + 3, r + 5, top + 9],                      # touches the right edge exactly: x0 == width, kept
        [left + 8, b, left + 20, b + 4],                   # touches the bottom edge exactly: y0 == height, kept
        [left + 30, top + 10, left + 33.5, top + 12.25],   # small, fractional, ignore category
    ]
    classes = [0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 2, 3, IGNORE]
    return boxes, classes


def _images(h=H0, w=W0, L=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (L, 3, h, w), generator=g, dtype=torch.uint8).float() / 255


def _same(boxes_t, classes_t, boxes_l, classes_l):
    assert classes_t.tolist() == classes_l
    assert boxes_t.shape == (len(boxes_l), 4)
    if boxes_l:
        assert torch.equal(boxes_t, torch.tensor(boxes_l, dtype=torch.float32)), (boxes_t, boxes_l)


def test_annotation_semantics_of_every_transform():
    import future_od.datasets.transforms as T
    images = _images()
    dropped = kept = 0

    # fixed crops: centre crop 40 x 70 of 60 x 100 -> top 10, left 15
    boxes, classes = _case_boxes(15, 10, 70, 40)
    bt, ct = torch.tensor(boxes, dtype=torch.float32), torch.tensor(classes)
    im, b, c = T.JointCenterCrop((40, 70))(images, bt.clone(), ct.clone())
    rb, rc = ref_crop(boxes, classes, 15, 10, 70, 40)
    _same(b, c, rb, rc)
    assert torch.equal(im, images[..., 10:50, 15:85])
    kept += len(rc); dropped += len(classes) - len(rc)
    assert len(rc) == 9 and IGNORE in rc                      # 5 overlapping + 3 touching + the ignore box; 4 outside gone
    assert [x for x in rb if x[2] == 0.0] and [x for x in rb if x[0] == 70.0] and [x for x in rb if x[1] == 40.0]

    # the random crops draw a rectangle inside the frame; the same rule applies to whatever they draw
    for t in (T.JointRandomCrop((40, 70)), T.RandomSizedCrop(0.5, 1.0), T.CenterBiasedRandomSizedCrop(0.5, 0.9)):
        for seed in range(4):
            plan = t.plan(H0, W0, random.Random(seed))
            top, left, ch, cw = plan.rect
            assert 0 <= top <= H0 - ch and 0 <= left <= W0 - cw
            if isinstance(t, T.RandomSizedCrop):               # ONE scale for both sides
                scale = random.Random(seed).uniform(t._min_scale, t._max_scale)
                assert (ch, cw) == (int(H0 * scale), int(W0 * scale))
            boxes, classes = _case_boxes(left, top, cw, ch)
            bt, ct = torch.tensor(boxes, dtype=torch.float32), torch.tensor(classes)
            random.seed(seed)
            im, b, c = t(images, bt, ct)
            assert tuple(im.shape[-2:]) == (ch, cw) and torch.equal(im, images[..., top:top + ch, left:left + cw])
            rb, rc = ref_crop(boxes, classes, left, top, cw, ch)
            _same(b, c, rb, rc)
            kept += len(rc); dropped += len(classes) - len(rc)

    # resize, flip, size filter, no-op, on the boxes that lie inside the frame
    boxes, classes = _case_boxes(15, 10, 70, 40)
    bt, ct = torch.tensor(boxes, dtype=torch.float32), torch.tensor(classes)
    im, b, c = T.JointResize((45, 64))(images, bt, ct)
    assert tuple(im.shape) == (2, 3, 45, 64)
    assert torch.equal(im, F.interpolate(images, size=(45, 64), mode="bilinear", align_corners=False))
    _same(b, c, *ref_resize(boxes, classes, W0, H0, 64, 45))
    im, b, c = T.JointHorizontalFlip(1.0)(images, bt, ct)
    assert torch.equal(im, images.flip(-1))
    _same(b, c, *ref_flip(boxes, classes, W0))
    im, b, c = T.JointHorizontalFlip(0.0)(images, bt, ct)
    assert im is images and torch.equal(b, bt)
    im, b, c = T.SizeFilter(0.01)(images, bt, ct)
    rb, rc = ref_size_filter(boxes, classes, W0, H0, 0.01)
    _same(b, c, rb, rc)
    assert 0 < len(rc) < len(classes) and IGNORE not in rc    # the 3.5 x 2.25 box is 0.13 % of the frame
    kept += len(rc); dropped += len(classes) - len(rc)
    im, b, c = T.JointNoOpTransform()(images, bt, ct)
    assert im is images and b is bt and c is ct
    assert torch.equal(T.ImageRemap()(torch.tensor([0, 51, 255], dtype=torch.uint8)), torch.tensor([0.0, 0.2, 1.0]))
    assert kept > 0 and dropped > 0

    # the composition the loaders use, step by step
    random.seed(7)
    compose = T.JointCompose([T.RandomSizedCrop(0.5, 1.0), T.JointResize((32, 48)), T.JointHorizontalFlip(1.0),
                              T.SizeFilter(0.002)])
    top, left, ch, cw = T.RandomSizedCrop(0.5, 1.0).plan(H0, W0, random.Random(7)).rect
    boxes, classes = _case_boxes(left, top, cw, ch)
    im, b, c = compose(images, torch.tensor(boxes, dtype=torch.float32), torch.tensor(classes))
    rb, rc = ref_crop(boxes, classes, left, top, cw, ch)
    rb, rc = ref_resize(rb, rc, cw, ch, 48, 32)
    rb, rc = ref_flip(rb, rc, 48)
    rb, rc = ref_size_filter(rb, rc, 48, 32, 0.002)
    _same(b, c, rb, rc)
    assert tuple(im.shape) == (2, 3, 32, 48) and 0 < len(rc) < len(classes)


def _run_plan(plan, images, boxes, classes):
    """A plan executed on the host: crop by slicing, F.interpolate, flip(-1)."""
    top, left, h, w = plan.rect
    im = images[..., top:top + h, left:left + w]
    if plan.size != (h, w):
        im = F.interpolate(im, size=plan.size, mode="bilinear", align_corners=False)
    if plan.flip:
        im = im.flip(-1)
    b, c = plan.annotate(boxes, classes)
    return im, b, c


def test_plan_equals_call():
    import future_od.datasets.transforms as T
    h0, w0 = 90, 160
    images = _images(h0, w0, L=3, seed=1)
    composes = {
        "train": T.JointCompose([T.RandomSizedCrop(0.5, 1.0), T.JointResize((448, 800))]),
        "val": T.JointCompose([T.JointCenterCrop((48, 80))]),
        "flip": T.JointCompose([T.SizeFilter(0.001), T.CenterBiasedRandomSizedCrop(0.6, 1.0),
                                T.JointRandomCrop((40, 64)), T.JointNoOpTransform(), T.JointResize((56, 72)),
                                T.JointHorizontalFlip(0.5)]),
        "select": T.JointCompose([T.RandomSelect(T.JointCenterCrop((60, 100)), T.RandomSizedCrop(0.5, 0.8), p=0.5),
                                  T.JointResize((32, 40)), T.JointHorizontalFlip(0.5), T.SizeFilter(0.004)]),
    }
    flips = set()
    for name, t in composes.items():
        for seed in range(6 if name in ("flip", "select") else 3):
            g = torch.Generator().manual_seed(100 + seed)
            n = 12
            xy = torch.rand(n, 2, generator=g) * torch.tensor([w0 - 20.0, h0 - 12.0])
            boxes = torch.cat([xy, xy + torch.rand(n, 2, generator=g) * torch.tensor([60.0, 40.0]) + 1], dim=1)
            classes = torch.randint(0, 9, (n,), generator=g)
            random.seed(seed)
            im_c, b_c, c_c = t(images, boxes.clone(), classes.clone())
            plan = t.plan(h0, w0, random.Random(seed))
            im_p, b_p, c_p = _run_plan(plan, images, boxes.clone(), classes.clone())
            assert tuple(im_c.shape[-2:]) == plan.size
            assert torch.equal(im_c, im_p), (name, seed, plan)
            assert torch.equal(b_c, b_p) and torch.equal(c_c, c_p), (name, seed, plan)
            top, left, h, w = plan.rect
            assert 0 <= top and top + h <= h0 and 0 <= left and left + w <= w0
            assert plan.row() == (top, left, h, w, int(plan.flip))
            if name in ("flip", "select"):
                flips.add(plan.flip)
    assert flips == {True, False}
    assert composes["val"].plan(h0, w0).rect == (21, 40, 48, 80) and composes["val"].plan(h0, w0).size == (48, 80)
    # at the camera's size: the centre crop the validation loader takes
    assert T.JointCenterCrop((896, 1600)).plan(900, 1600).row() == (2, 0, 896, 1600, 0)


def test_unplannable_composes_raise():
    import future_od.datasets.transforms as T
    rng = random.Random(0)
    bad = {
        "JointResize": T.JointCompose([T.JointResize((32, 48)), T.JointResize((16, 24))]),
        "JointCenterCrop": T.JointCompose([T.JointResize((32, 48)), T.JointCenterCrop((16, 24))]),
        "RandomSizedCrop": T.JointCompose([T.JointHorizontalFlip(0.0), T.RandomSizedCrop(0.5, 1.0)]),
        "JointHorizontalFlip": T.JointCompose([T.JointHorizontalFlip(0.0), T.JointHorizontalFlip(0.0)]),
    }
    for step, t in bad.items():
        with pytest.raises(ValueError, match=step):
            t.plan(60, 100, rng)
    with pytest.raises(ValueError, match="JointResize"):
        T.JointCompose([T.JointCompose([T.JointResize((32, 48))]), T.JointResize((16, 24))]).plan(60, 100, rng)
    with pytest.raises(ValueError, match="nearest"):
        T.JointResize((32, 48), interpolation="nearest").plan(60, 100, rng)
    with pytest.raises(ValueError, match="leaves"):                       # a crop larger than the frame would pad
        T.JointCenterCrop((64, 96)).plan(60, 100, rng)
    with pytest.raises(ValueError, match="leaves"):
        T.JointCenterCrop((64, 96))(_images(), torch.zeros(0, 4), torch.zeros(0, dtype=torch.int64))
    # ... while the per-sample form of a two-resize compose still runs: it resamples twice
    im, _, _ = bad["JointResize"](_images(), torch.zeros(0, 4), torch.zeros(0, dtype=torch.int64))
    assert tuple(im.shape[-2:]) == (16, 24)


def _raw_batch(B, L, h, w, seed, max_boxes=12):
    from future_od.datasets.synthetic import make_batch
    batch = make_batch(B, L, h, w, seed=seed, max_boxes=max_boxes, min_boxes=6, raw_frames=True)
    assert batch["video"].dtype == torch.uint8 and int(batch["video"].max()) > 200
    # a few ignore boxes, as the reference's datasets emit them
    batch["ignore_boxes"][:, 0] = torch.tensor([2.0, 3.0, 30.0, 20.0])
    batch["ignore_boxes"][:, 1] = torch.tensor([w - 9.0, h - 7.0, w - 1.0, h - 1.0])
    return batch


def test_device_transform_host_half_on_dense_batches():
    import future_od.datasets.transforms as T
    from future_od.datasets.synthetic import MAX_NUM_OBJECTS
    from future_od.utils.augment import DeviceJointTransform
    h0, w0, B = 90, 160, 4
    t = T.JointCompose([T.RandomSizedCrop(0.5, 0.7), T.JointResize((64, 96)), T.JointHorizontalFlip(0.5),
                        T.SizeFilter(0.004)])
    dropped = 0
    dt = DeviceJointTransform(t, seed=5, rank=0)
    for index in range(3):
        batch = _raw_batch(B, 2, h0, w0, seed=40 + index)
        before = {k: v.clone() for k, v in batch.items() if isinstance(v, torch.Tensor)}
        out = dt.host(batch)
        assert all(torch.equal(before[k], batch[k]) for k in before)                  # the loader's batch is not touched
        assert out["video"] is batch["video"] and out["plans"].dtype == torch.int32 and out["plans"].shape == (B, 5)
        assert out["boxes"].shape == (B, MAX_NUM_OBJECTS, 4) and out["classes"].dtype == torch.int64
        for b in range(B):
            rows = batch["active"][b].bool()
            random.setstate(dt.sample_rng(index, b).getstate())
            images = batch["video"][b].float() / 255
            im, bx, cl = t(images, batch["boxes"][b][rows], batch["classes"][b][rows])
            n = bx.shape[0]
            dropped += int(rows.sum()) - n
            want_b, want_c = torch.zeros(MAX_NUM_OBJECTS, 4), torch.zeros(MAX_NUM_OBJECTS, dtype=torch.int64)
            want_a = torch.zeros(MAX_NUM_OBJECTS, dtype=torch.int64)
            want_b[:n], want_c[:n], want_a[:n] = bx, cl, 1
            assert torch.equal(out["boxes"][b], want_b) and torch.equal(out["classes"][b], want_c)
            assert torch.equal(out["active"][b], want_a)
            random.setstate(dt.sample_rng(index, b).getstate())
            ig = batch["ignore_boxes"][b][:2]
            _, ig_want, _ = t(images, ig, torch.zeros(2, dtype=torch.int64))
            assert torch.equal(out["ignore_boxes"][b, :ig_want.shape[0]], ig_want)
            assert not out["ignore_boxes"][b, ig_want.shape[0]:].any()
            plan = t.plan(h0, w0, dt.sample_rng(index, b))
            assert out["plans"][b].tolist() == list(plan.row()) and tuple(im.shape[-2:]) == plan.size == (64, 96)
        host = out["_host_annotations"]
        assert set(host) == {"active", "boxes", "classes"}
        assert all(host[k] is out[k] for k in host)
    assert dropped > 0
    # one seed, one stream of plans; another rank, other rectangles
    batch = _raw_batch(B, 2, h0, w0, seed=1)
    a, b_, c = (DeviceJointTransform(t, seed=5, rank=r) for r in (0, 0, 1))
    pa = [a.host(batch)["plans"] for _ in range(3)]
    pb = [b_.host(batch)["plans"] for _ in range(3)]
    pc = [c.host(batch)["plans"] for _ in range(3)]
    assert all(torch.equal(x, y) for x, y in zip(pa, pb))
    assert not torch.equal(pa[0], pa[1]) and not torch.equal(pa[0], pc[0])
    assert torch.equal(a.host(batch, index=1)["plans"], pa[1])                        # (seed, rank, batch index) decide
    with pytest.raises(ValueError, match="uint8"):
        a.host({**batch, "video": batch["video"].float()})
    with pytest.raises(ValueError, match="output size"):                              # no common size without a resize
        DeviceJointTransform(T.RandomSizedCrop(0.5, 1.0)).host(batch)


def test_loaders_honour_random_aug():
    import future_od.datasets.transforms as T
    from future_od.datasets import nu_scenes
    from future_od.datasets.synthetic import make_batch
    from future_od.utils.augment import DeviceJointTransform
    from future_od.utils.prefetch import DevicePrefetcher
    from runs._loader import get_nuim_loaders, get_nusc_loaders
    args = SimpleNamespace(distributed=True, world_size=2, world_rank=1)
    offsets = [-1.0, -0.5, 0]
    # the default path: no transform, float clips at img_size, today's seed rule
    train, val = get_nusc_loaders((32, 48), offsets=offsets, config={}, args=args, train_batch_size=4, steps_per_epoch=2,
                                  val_steps=1)
    assert not hasattr(train, "device_transform") and not hasattr(val["val"], "device_transform")
    for loader, seed in ((train, 1234), (val["val"], 99991)):
        for i, got in enumerate(loader):
            want = make_batch(2, 3, 32, 48, seed=seed + 7919 * (i * 2 + 1), max_boxes=40)
            want["temporal_offsets"] = torch.tensor(offsets).repeat(2, 1)
            assert got["video"].dtype == torch.float32 and got["video"].shape == (2, 3, 3, 32, 48)
            assert set(got) == set(want)
            for k, v in want.items():
                if isinstance(v, torch.Tensor):
                    assert torch.equal(got[k], v), k
    assert len(list(DevicePrefetcher(train, "cpu"))) == 2                             # still a plain batch mover

    # with a transform: raw uint8 frames at the raw size, boxes in those coordinates, a device transform on board
    aug = T.RandomSizedCrop(0.5, 1.0)
    train, val = get_nusc_loaders((32, 48), offsets=offsets, config={}, args=args, train_batch_size=4, random_aug=aug,
                                  steps_per_epoch=2, val_steps=1, raw_size=(45, 80))
    batches = list(train)
    assert len(batches) == 2 and train.dataset.size == (32, 48) and train.dataset.raw_size == (45, 80)
    for b in batches:
        assert b["video"].dtype == torch.uint8 and b["video"].shape == (2, 3, 3, 45, 80)
        act = b["active"].bool()
        assert float(b["boxes"][act][:, 2].max()) <= 80 and float(b["boxes"][act][:, 3].max()) <= 45
    assert float(max(b["boxes"][..., 2].max() for b in batches)) > 48                 # raw coordinates, not img_size ones
    dt = train.device_transform
    assert isinstance(dt, DeviceJointTransform) and dt.rank == 1
    steps = dt.joint_transform.transforms
    assert steps[0] is aug and isinstance(steps[1], T.JointResize) and steps[1]._size == [32, 48]
    vsteps = val["val"].device_transform.joint_transform.transforms
    assert len(vsteps) == 1 and isinstance(vsteps[0], T.JointCenterCrop) and (vsteps[0].th, vsteps[0].tw) == (32, 48)
    out = dt.host(batches[0])
    assert out["plans"].shape == (2, 5) and float(out["boxes"][..., 2].max()) <= 48
    with pytest.raises(RuntimeError, match="GPU"):
        DevicePrefetcher(train, "cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        list(DevicePrefetcher(val["val"], "cpu"))
    # the camera's size is the default raw size; the NuImages factory takes the same arguments
    train, _ = get_nuim_loaders((448, 800), offsets=[0], config={}, args=SimpleNamespace(distributed=False),
                                train_batch_size=1, random_aug=aug, steps_per_epoch=1, val_steps=1)
    assert train.dataset.raw_size == nu_scenes.ORIGINAL_IMSIZE == (900, 1600)


def test_clip_crop_resize_has_no_cpu_fallback():
    from future_od.native import lib as L
    from future_od.native import ops
    with pytest.raises(L.FodError):
        ops.clip_crop_resize(torch.zeros(1, 1, 3, 8, 8, dtype=torch.uint8), torch.zeros(1, 5, dtype=torch.int32), (4, 4),
                             torch.zeros(3), torch.ones(3))
    assert "fod_clip_crop_resize" in L.FAST and L.ABI_VERSION >= 6          # the entry point came with ABI 6
    rc = L.LIB.fod_clip_crop_resize(None, None, 1, 1, 3, 8, 8, 4, 4, 192, 192, None, None, None, None)
    assert rc != 0 and "null" in L.last_error()
