"""Photometric augmentation, the parts that need no GPU: the entry point as the binding reads it from include/fod_ext.h
and its argument checks, the CPU form of JointPhotometricDistortion against a float64 restatement of the definition
(tests/photometric_cases.py), its exact anchors, its draws, how it composes into plans, the `photo` rows of
DeviceJointTransform.host and the loaders' `photometric` keyword."""
import os
import random
import re
from types import SimpleNamespace

import pytest
import torch

import photometric_cases as PC
from future_od.native import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, LONG = "pointer", "int", "long"
ENTRY = "fod_clip_crop_resize_photo"

# The CPU form (float32) against the float64 restatement on _pixels(): the largest distance in normalised units, per
# row of PC.ROWS, as measured on the CPU (test_cpu_form_against_float64 prints each figure; `pytest -s` shows them).
# The figure that came with the definition is 3.6e-6 on other pixels; the limit the tests hold the distance to is 1e-4.
MEASURED_F32_TO_F64 = {
    "brightness": 6.65e-08,
    "darker": 1.33e-07,
    "contrast": 1.31e-07,
    "contrast down": 1.31e-07,
    "saturation": 3.16e-06,
    "desaturation": 1.50e-06,
    "hue": 4.21e-06,
    "hue back": 4.51e-06,
    "all, contrast after": 5.30e-06,
    "all, contrast first": 1.79e-06,
}
LIMIT = 1e-4


def _pixels():
    """A float32 clip [2, 3, 96, 176] in 0..1: uint8 noise / 255 with the structured blocks on top."""
    return PC.structured_frames(2, 96, 176, seed=7).float() / 255


def measure(name):
    import future_od.datasets.transforms as T
    p = _pixels()
    got = T.photometric(p, PC.ROWS[name])
    assert got.dtype == torch.float32 and got.shape == p.shape
    want = PC.restated(p, PC.ROWS[name], torch.float64)
    return float((PC.normalise(got.double()) - PC.normalise(want)).abs().max())


# ---- ABI and binding ---------------------------------------------------------------------------------------------------
def test_prototype_is_read_from_the_second_header():
    assert abi.EXT_PROTOTYPES[ENTRY] == (I, [P, P, I, I, I, I, I, I, I, LONG, LONG, P, P, P, P, P])
    assert abi.EXT_PROTOTYPES[ENTRY][1] == abi.PROTOTYPES["fod_clip_crop_resize"][1][:-1] + [P, P]   # photo, then the stream
    assert ENTRY not in abi.PROTOTYPES and ENTRY not in abi.served(abi.PROTOTYPES)
    assert ENTRY not in open(abi.HEADER_PATH).read()
    from future_od.native import lib as L
    assert ENTRY in L.EXT_SIGNATURES and ENTRY in L._ENTRY and ENTRY not in L.SIGNATURES and ENTRY not in L.FAST
    fn = getattr(L.LIB, ENTRY)
    assert fn.restype is abi.CTYPE[I] and list(fn.argtypes) == [abi.CTYPE[k] for k in abi.EXT_PROTOTYPES[ENTRY][1]]


def test_abi_version_moved_with_the_entry_point():
    from future_od.native import lib as L
    hdr = open(os.path.join(ROOT, "include", "fod.h")).read()
    assert int(re.search(r"#define FOD_ABI_VERSION (\d+)", hdr).group(1)) == L.ABI_VERSION == L.LIB.fod_abi_version() >= 12


def test_arguments_are_refused_before_any_launch():
    """The non-null 'pointers' are the address 1: a launch would fault, so a clean non-zero return is the check itself."""
    from future_od.native import lib as L
    with pytest.raises(L.FodError, match="clip_crop_resize_photo"):
        L.call(ENTRY, None, None, 1, 1, 3, 8, 8, 4, 4, 192, 192, None, None, None, None, None)
    assert "null" in L.last_error()
    good = dict(src=1, dst=16, plans=1, mean=1, std=1, photo=1)
    for missing in good:                                                  # each pointer in turn
        a = {**good, missing: None}
        rc = getattr(L.LIB, ENTRY)(a["src"], a["dst"], 1, 1, 3, 8, 8, 4, 4, 192, 192, a["plans"], a["mean"], a["std"],
                                   a["photo"], None)
        assert rc != 0 and "clip_crop_resize_photo" in L.last_error() and "null" in L.last_error(), missing
    for c in (2, 1, 4, 0):
        rc = getattr(L.LIB, ENTRY)(1, 16, 1, 1, c, 8, 8, 4, 4, 64 * c, 64 * c, 1, 1, 1, 1, None)
        assert rc != 0 and "three planes" in L.last_error(), c
    for bad in ((0, 1, 3, 8, 8, 4, 4, 192, 192), (1, 1, 3, 8, 8, 0, 4, 192, 192), (1, 1, 3, 8, 8, 4, 4, 100, 192),
                (1, 1, 3, 0, 8, 4, 4, 192, 192)):
        assert getattr(L.LIB, ENTRY)(1, 16, *bad, 1, 1, 1, 1, None) != 0, bad
    assert getattr(L.LIB, ENTRY)(1, 8, 1, 1, 3, 8, 8, 4, 4, 192, 192, 1, 1, 1, 1, None) != 0 and "aligned" in L.last_error()


def test_wrapper_has_no_cpu_fallback():
    from future_od.native import lib as L
    from future_od.native import ops
    with pytest.raises(L.FodError, match="no CPU fallback"):
        ops.clip_crop_resize_photo(torch.zeros(1, 1, 3, 8, 8, dtype=torch.uint8), torch.zeros(1, 5, dtype=torch.int32),
                                   (4, 4), torch.zeros(3), torch.ones(3), torch.zeros(1, 5))


# ---- the CPU form, f32 against f64 ----------------------------------------------------------------------------------------
def test_every_stage_and_both_orders_are_covered():
    rows = PC.ROWS
    assert set(MEASURED_F32_TO_F64) == set(rows)
    active = lambda r: (r[0] != 0, r[1] != 1, r[2] != 1, r[3] != 0)
    for stage in range(4):                                                # each stage alone
        assert any(active(r)[stage] and sum(active(r)) == 1 for r in rows.values()), stage
    both = [r for r in rows.values() if all(active(r))]
    assert {r[4] for r in both} == {0.0, 1.0}
    px = _pixels()
    r, g, b = px[:, 0], px[:, 1], px[:, 2]
    for what in ((r == g) & (g == b) & (r > 0) & (r < 1), (r == 0) & (g == 0) & (b == 0), (r == 1) & (g == 0) & (b == 0),
                 (r == 0) & (g == 1) & (b == 0), (r == 0) & (g == 0) & (b == 1), (r == g) & (g != b), (g == b) & (r != g)):
        assert int(what.sum()) >= 64                                       # the structured blocks are there


@pytest.mark.parametrize("name", list(PC.ROWS))
def test_cpu_form_against_float64(name):
    err = measure(name)
    print(f"\n{name}: f32 CPU form to f64 restatement, max {err:.3e} (recorded {MEASURED_F32_TO_F64[name]:.3e})")
    assert err <= LIMIT, err
    recorded = MEASURED_F32_TO_F64[name]
    assert 0.5 * recorded <= err <= 2.0 * recorded, (name, err, recorded)    # the table above is current


# ---- exact anchors -----------------------------------------------------------------------------------------------------
def test_exact_anchors():
    import future_od.datasets.transforms as T
    px = _pixels()
    for first in (0.0, 1.0, 7.0):
        assert T.photometric(px, (0.0, 1.0, 1.0, 0.0, first)) is px
        assert torch.equal(PC.restated(px, (0.0, 1.0, 1.0, 0.0, first), torch.float32), px)
    assert torch.equal(T.photometric(px, (float("nan"), float("inf"), float("-inf"), float("nan"), 0.0)), px)
    assert T.sanitise_photo_row((5.0, -3.0, 1e30, -7.0, float("nan"))) == (1.0, 0.0, 4.0, 0.0, True)
    assert T.sanitise_photo_row((float("nan"),) * 5) == (0.0, 1.0, 1.0, 0.0, True)
    red = torch.tensor([1.0, 0.0, 0.0]).view(1, 3, 1, 1).expand(2, 3, 4, 5).contiguous()
    green = torch.tensor([0.0, 1.0, 0.0]).view(1, 3, 1, 1).expand(2, 3, 4, 5)
    for first in (0.0, 1.0):
        assert torch.equal(T.photometric(red, (0.0, 1.0, 1.0, 1 / 3, first)), green)
        assert torch.equal(PC.restated(red, (0.0, 1.0, 1.0, 1 / 3, first), torch.float32), green)
    grey = T.photometric(px, (0.0, 1.0, 0.0, 0.0, 0.0))
    v = px.amax(dim=1, keepdim=True).expand_as(px)
    assert torch.equal(grey, v)
    # a JointPhotometricDistortion that applies nothing returns the clip it was given; boxes and classes pass through
    t = T.JointPhotometricDistortion(p=0.0)
    boxes, classes = torch.tensor([[1.0, 2.0, 3.0, 4.0]]), torch.tensor([5])
    im, bx, cl = t(px, boxes, classes)
    assert im is px and bx is boxes and cl is classes


def test_normalised_clips_are_taken_with_mean_and_std():
    import future_od.datasets.transforms as T
    px = _pixels()
    t = T.JointPhotometricDistortion(p=1.0, pixel_mean=PC.MEAN.tolist(), pixel_std=PC.STD.tolist())
    random.seed(4)
    got, _, _ = t(PC.normalise(px), None, None)
    row = T.JointPhotometricDistortion(p=1.0).plan(96, 176, random.Random(4)).photo_row()
    want = PC.normalise(PC.restated(px, row, torch.float64))
    assert float((got.double() - want).abs().max()) < LIMIT


# ---- draws -------------------------------------------------------------------------------------------------------------
def test_call_and_plan_draw_the_same_row():
    """The CPU form and the float32 restatement run the same elementary float32 operations on the same row; 1e-6 (0..1
    scale) allows for nothing but a last bit, where another row moves whole percents."""
    import future_od.datasets.transforms as T
    px = _pixels()
    t = T.JointPhotometricDistortion(p=0.8)
    rows = set()
    for s in range(12):
        random.seed(s)
        got, _, _ = t(px, torch.zeros(0, 4), torch.zeros(0, dtype=torch.int64))
        row = t.plan(96, 176, random.Random(s)).photo_row()
        assert len(row) == 5 and all(isinstance(v, float) for v in row)
        assert float((got - PC.restated(px, row, torch.float32)).abs().max()) <= 1e-6, (s, row)
        rows.add(row)
    assert len(rows) == 12
    assert T.Plan(8, 8).photo_row() == (0.0, 1.0, 1.0, 0.0, 0.0) and T.Plan(8, 8).photo is None


def test_the_number_of_draws_does_not_depend_on_their_outcome():
    import future_od.datasets.transforms as T
    for s in range(20):
        states = []
        for p in (0.0, 0.3, 0.5, 1.0):
            rng = random.Random(s)
            T.JointPhotometricDistortion(p=p).plan(32, 48, rng)
            states.append(rng.getstate())
        nine = random.Random(s)
        for _ in range(9):
            nine.random()
        assert all(st == nine.getstate() for st in states), s


def test_drawn_values_lie_in_their_ranges_and_every_stage_is_drawn_both_ways():
    import future_od.datasets.transforms as T
    t = T.JointPhotometricDistortion(brightness_delta=0.2, contrast_range=(0.6, 1.7), saturation_range=(0.25, 2.0),
                                     hue_delta=0.1, p=0.5)
    neutral, lo, hi = (0.0, 1.0, 1.0, 0.0), (-0.2, 0.6, 0.25, -0.1), (0.2, 1.7, 2.0, 0.1)
    applied, skipped, firsts = [0] * 4, [0] * 4, set()
    for s in range(1000):
        row = t.plan(20, 30, random.Random(s)).photo_row()
        for i in range(4):
            assert lo[i] <= row[i] <= hi[i], (s, row)
            applied[i] += row[i] != neutral[i]
            skipped[i] += row[i] == neutral[i]
        firsts.add(row[4])
    assert all(300 < n < 700 for n in applied + skipped), (applied, skipped)
    assert firsts == {0.0, 1.0}


@pytest.mark.parametrize("kw", [dict(brightness_delta=-0.1), dict(brightness_delta=1.5), dict(contrast_range=(1.5, 0.5)),
                                dict(contrast_range=(-0.5, 1.0)), dict(saturation_range=(0.5, 4.5)),
                                dict(saturation_range=(1.0,)), dict(hue_delta=0.6), dict(hue_delta=-0.01), dict(p=1.5),
                                dict(pixel_mean=[0.5, 0.5, 0.5]), dict(pixel_mean=[0.5] * 3, pixel_std=[0.2, 0.0, 0.2])])
def test_bad_constructor_arguments_raise(kw):
    import future_od.datasets.transforms as T
    with pytest.raises(ValueError):
        T.JointPhotometricDistortion(**kw)


# ---- composition -------------------------------------------------------------------------------------------------------
def test_composition_with_the_geometric_steps():
    import future_od.datasets.transforms as T
    photo = T.JointPhotometricDistortion(p=1.0)
    boxes = torch.tensor([[5.0, 6.0, 40.0, 30.0], [50.0, 20.0, 90.0, 55.0], [0.0, 0.0, 8.0, 8.0]])
    classes = torch.tensor([1, 2, 3])
    for geometric in ([T.RandomSizedCrop(0.5, 0.9), T.JointResize((32, 48))], [T.RandomSizedCrop(0.5, 0.9)],
                      [T.RandomSizedCrop(0.6, 1.0), T.JointResize((24, 40)), T.JointHorizontalFlip(0.5), T.SizeFilter(0.01)]):
        for s in range(6):
            with_photo = T.JointCompose(geometric + [photo]).plan(60, 100, random.Random(s))
            without = T.JointCompose(geometric).plan(60, 100, random.Random(s))
            assert with_photo.row() == without.row() and with_photo.size == without.size
            assert with_photo.steps == without.steps                      # no annotation step of its own
            (b1, c1), (b2, c2) = with_photo.annotate(boxes, classes), without.annotate(boxes, classes)
            assert torch.equal(b1, b2) and torch.equal(c1, c2)
            assert without.photo is None and with_photo.photo is not None and with_photo.photo_row() != PC.NEUTRAL
    # per-pixel work commutes with a flip and a crop: both plan after it
    plan = T.JointCompose([photo, T.JointHorizontalFlip(1.0)]).plan(60, 100, random.Random(0))
    assert plan.flip and plan.photo is not None
    plan = T.JointCompose([photo, T.JointCenterCrop((30, 50))]).plan(60, 100, random.Random(0))
    assert plan.rect == (15, 25, 30, 50) and plan.photo is not None
    # ... but not with resampling, and a clip has one row
    with pytest.raises(ValueError, match="JointResize"):
        T.JointCompose([photo, T.JointResize((32, 48))]).plan(60, 100, random.Random(0))
    with pytest.raises(ValueError, match="JointResize"):
        T.JointCompose([T.RandomSizedCrop(0.5, 1.0), photo, T.JointHorizontalFlip(), T.JointResize((32, 48))]).plan(60, 100)
    with pytest.raises(ValueError, match="JointPhotometricDistortion"):
        T.JointCompose([photo, T.JointHorizontalFlip(), T.JointPhotometricDistortion()]).plan(60, 100, random.Random(0))
    # RandomSelect plans the branch it draws, with or without a photometric step
    select = T.RandomSelect(T.JointCompose([T.JointResize((32, 48)), photo]), T.JointResize((32, 48)), p=0.5)
    seen = {select.plan(60, 100, random.Random(s)).photo is not None for s in range(40)}
    assert seen == {True, False}
    assert T.has_photometric(select) and T.has_photometric(T.JointCompose([T.JointNoOpTransform(), select]))
    assert not T.has_photometric(T.JointCompose([T.RandomSizedCrop(0.5, 1.0), T.JointResize((32, 48))]))


# ---- DeviceJointTransform.host -----------------------------------------------------------------------------------------
def _raw_batch(B, L, h, w, seed):
    from future_od.datasets.synthetic import make_batch
    return make_batch(B, L, h, w, seed=seed, max_boxes=12, min_boxes=6, raw_frames=True)


def test_host_half_adds_one_row_per_clip():
    import future_od.datasets.transforms as T
    from future_od.utils.augment import DeviceJointTransform
    h0, w0, B = 45, 80, 3
    geometric = [T.RandomSizedCrop(0.5, 0.9), T.JointResize((32, 48))]
    t = T.JointCompose(geometric + [T.JointPhotometricDistortion(p=0.7)])
    dt, plain = DeviceJointTransform(t, seed=5, rank=1), DeviceJointTransform(T.JointCompose(geometric), seed=5, rank=1)
    seen = []
    for index in range(3):
        batch = _raw_batch(B, 2, h0, w0, seed=60 + index)
        out, ref = dt.host(batch), plain.host(batch)
        assert out["photo"].dtype == torch.float32 and out["photo"].shape == (B, 5) and not out["photo"].is_cuda
        assert "photo" not in ref and set(out) == set(ref) | {"photo"}
        for k in ("plans", "boxes", "classes", "active", "ignore_boxes"):    # the geometric half does not notice
            assert torch.equal(out[k], ref[k]), k
        assert "photo" not in out["_host_annotations"]
        for b in range(B):
            row = t.plan(h0, w0, dt.sample_rng(index, b)).photo_row()
            assert torch.equal(out["photo"][b], torch.tensor(row, dtype=torch.float32))
        seen.append(out["photo"])
        assert torch.equal(dt.host(batch, index=index)["photo"], out["photo"])         # (seed, rank, index, sample) decide
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[0][0], seen[0][1])
    assert not torch.equal(DeviceJointTransform(t, seed=5, rank=0).host(batch, index=0)["photo"], seen[0])
    assert not torch.equal(DeviceJointTransform(t, seed=6, rank=1).host(batch, index=0)["photo"], seen[0])
    # label-free frames carry the rows too
    free = {k: v for k, v in _raw_batch(B, 2, h0, w0, seed=60).items() if k not in ("boxes", "classes", "active")}
    out, ref = dt.host(free, index=0), plain.host(free, index=0)
    assert torch.equal(out["photo"], seen[0]) and "box_map" in out and "photo" not in ref
    assert set(out) == set(ref) | {"photo"} and torch.equal(out["plans"], ref["plans"])
    # a RandomSelect whose drawn branch has no photometric step: the neutral row
    select = T.RandomSelect(T.JointCompose([T.JointResize((32, 48)), T.JointPhotometricDistortion(p=1.0)]),
                            T.JointResize((32, 48)), p=0.5)
    rows = torch.cat([DeviceJointTransform(select, seed=1).host(free, index=i)["photo"] for i in range(8)])
    is_neutral = (rows[:, :4] == torch.tensor(PC.NEUTRAL[:4])).all(dim=1)
    assert bool(is_neutral.any()) and not bool(is_neutral.all())


# ---- loader keyword ----------------------------------------------------------------------------------------------------
def test_loaders_take_a_photometric_step():
    import inspect
    import future_od.datasets.transforms as T
    from runs._loader import get_nuim_loaders, get_nusc_loaders
    args, aug, photo = SimpleNamespace(distributed=False), T.RandomSizedCrop(0.5, 1.0), T.JointPhotometricDistortion()
    for factory in (get_nusc_loaders, get_nuim_loaders):
        assert inspect.signature(factory).parameters["photometric"].default is None
        train, val = factory((32, 48), offsets=[-0.5, 0], config={}, args=args, train_batch_size=2, random_aug=aug,
                             steps_per_epoch=2, val_steps=1, raw_size=(45, 80), photometric=photo)
        steps = train.device_transform.joint_transform.transforms
        assert len(steps) == 3 and steps[0] is aug and isinstance(steps[1], T.JointResize) and steps[1]._size == [32, 48]
        assert steps[2] is photo and train.device_transform.photometric
        vsteps = val["val"].device_transform.joint_transform.transforms
        assert len(vsteps) == 1 and isinstance(vsteps[0], T.JointCenterCrop) and not val["val"].device_transform.photometric
        out = train.device_transform.host(next(iter(train)))
        assert out["photo"].shape == (2, 5) and "photo" not in val["val"].device_transform.host(next(iter(val["val"])))
        with pytest.raises(ValueError, match="random_aug"):
            factory((32, 48), offsets=[0], config={}, args=args, train_batch_size=2, photometric=photo)
        train, _ = factory((32, 48), offsets=[0], config={}, args=args, train_batch_size=2, random_aug=aug,
                           raw_size=(45, 80))
        assert len(train.device_transform.joint_transform.transforms) == 2 and not train.device_transform.photometric
    assert list(inspect.signature(get_nusc_loaders).parameters)[-1] == "photometric"

