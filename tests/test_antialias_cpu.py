"""Antialiased downscaling, the parts that need no GPU: the restated definition (tests/antialias_cases.py) against
torch's float64 `interpolate(antialias=True)`, the recorded limits re-measured, the entry point as the binding reads it
and its refusals before any launch, `JointResize(antialias=True)` on the CPU, plans / boxes / draws with and without
the flag, `uses_antialias`, and the loaders' keyword."""
import inspect
import math
import random
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import antialias_cases as AC
import photometric_cases as PC
from future_od.native import abi

P, I, LONG = "pointer", "int", "long"
ENTRY = "fod_clip_crop_resize_aa"
IDS = [c["name"] for c in AC.CASES]


def torch_aa(crop_u8, size, dtype):
    return F.interpolate(crop_u8.to(dtype), size=size, mode="bilinear", align_corners=False, antialias=True)


def cpu_form_f32(crop_u8, size):
    """torch's float32 CPU evaluation of the whole chain: its antialiased resize, / 255, the normalisation."""
    return AC.normalise(torch_aa(crop_u8, size, torch.float32) / 255)


def measure(case):
    """The case's largest distance, on normalised outputs, between the float32 CPU form and the float64 restatement."""
    u8 = AC.view(AC.source(case), case)
    return float((AC.expected(case, u8, None, cpu_form_f32).double() - AC.expected(case, u8, torch.float64)).abs().max())


def measure_photo(name):
    case = AC.PHOTO_CASE
    u8 = AC.source(case)
    f32 = AC.expected(case, u8, None, lambda crop, size: PC.normalise(
        PC.restated(torch_aa(crop, size, torch.float32) / 255, PC.ROWS[name], torch.float32)))
    f64 = AC.expected(case, u8, None, lambda crop, size: PC.normalise(
        PC.restated(AC.sample(crop, size, torch.float64) / 255, PC.ROWS[name], torch.float64)))
    return float((f32.double() - f64).abs().max())


def e2e_transform(antialias=True, photometric=None):
    import future_od.datasets.transforms as T
    return T.JointCompose([T.RandomSizedCrop(0.5, 1.0), T.JointResize(AC.E2E["size"], antialias=antialias),
                           T.JointHorizontalFlip(0.5)] + ([photometric] if photometric is not None else []))


def e2e_batch():
    from future_od.datasets.synthetic import make_batch
    return make_batch(AC.E2E["B"], AC.E2E["L"], *AC.E2E["raw"], seed=77, max_boxes=12, min_boxes=6, raw_frames=True)


def e2e_cpu(dt, batch, index=0):
    """-> per sample (images f32 [L, 3, H, W], boxes, classes, f64 restatement of the sample's plan): the per-sample CPU
    transform on the normalised float clip, drawing what DeviceJointTransform.host draws for (index, sample)."""
    out, before = [], random.getstate()
    h0, w0 = AC.E2E["raw"]
    for b in range(AC.E2E["B"]):
        rows = batch["active"][b].bool()
        random.setstate(dt.sample_rng(index, b).getstate())
        clip = AC.normalise(batch["video"][b].float() / 255)
        images, boxes, classes = dt.joint_transform(clip, batch["boxes"][b][rows], batch["classes"][b][rows])
        plan = dt.joint_transform.plan(h0, w0, dt.sample_rng(index, b))
        top, left, h, w = plan.rect
        exact = AC.restated(batch["video"][b][..., top:top + h, left:left + w], plan.size, torch.float64)
        out.append((images, boxes, classes, exact.flip(-1) if plan.flip else exact))
    random.setstate(before)                   # the per-sample form draws from the global generator: leave it as it was
    return out


def measure_e2e():
    from future_od.utils.augment import DeviceJointTransform
    dt = DeviceJointTransform(e2e_transform(), seed=AC.E2E["seed"])
    return max(float((im.double() - exact).abs().max()) for im, _, _, exact in e2e_cpu(dt, e2e_batch()))


def _check_recorded(recorded, distance, what):
    print(f"\n{what}: f32 CPU form to f64 restatement, max {distance:.3e}; recorded limit {recorded:.3e} "
          f"= {recorded / distance:.2f} x")
    assert 3 * distance <= recorded <= 6 * distance, (what, distance, recorded)


# ---- the definition ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", AC.CASES, ids=IDS)
def test_restatement_is_torchs_float64_antialiased_resize(case):
    u8 = AC.view(AC.source(case), case)
    got = AC.expected(case, u8, None, lambda crop, size: AC.sample(crop, size, torch.float64))
    want = AC.expected(case, u8, None, lambda crop, size: torch_aa(crop, size, torch.float64))
    assert got.shape == (case["B"], case["L"], case["C"], *case["size"])
    assert float((got - want).abs().max()) <= 1e-12                  # on the 0..255 values themselves


def test_anchors_of_the_definition():
    g = torch.Generator().manual_seed(5)
    u8 = torch.randint(0, 256, (2, 3, 30, 50), generator=g, dtype=torch.uint8)
    for dtype in (torch.float32, torch.float64):
        assert torch.equal(AC.sample(u8, (30, 50), dtype), u8.to(dtype))           # an unchanged size copies the source
    up = AC.sample(u8[..., :11, :13], (22, 26), torch.float64)                       # enlarging: plain bilinear's values
    plain = F.interpolate(u8[..., :11, :13].double(), size=(22, 26), mode="bilinear", align_corners=False)
    assert float((up - plain).abs().max()) <= 1e-10
    for n_in, n_out, count in ((1600, 800, 4), (900, 448, 5), (450, 448, 3)):        # taps per axis at the product's ratios
        assert int((AC.taps(n_in, n_out, torch.float64) > 0).sum(dim=1).max()) <= count
        assert int((AC.taps(n_in, n_out, torch.float64) != 0).sum(dim=1).max()) >= 2
    white = AC.restated(torch.full((3, 50, 90), 255, dtype=torch.uint8), (24, 44), torch.float64)
    assert float((white - ((1 - AC.MEAN.double()) / AC.STD.double()).view(3, 1, 1)).abs().max()) <= 1e-12
    assert AC.clamped((-5, 70, 30, 50, 0), 45, 80) == (0, 30, 30, 50, 0)
    assert AC.clamped((7, 11, 4000, -3, 2), 45, 80) == (0, 11, 45, 1, 1)


def test_cases_cover_what_they_are_there_for():
    ratios = []
    for case in AC.CASES:
        H, W = case["size"]
        assert case["H0"] <= AC.MAX_RATIO * H and case["W0"] <= AC.MAX_RATIO * W, case["name"]
        for plan in case["plans"]:
            _, _, h, w, _ = AC.clamped(plan, case["H0"], case["W0"])
            ratios += [h / H, w / W]
    assert min(ratios) <= 0.5 and max(ratios) == 4 and any(r == 1 for r in ratios)
    assert any(1.5 < r < 1.7 for r in ratios) and any(3 < r < 3.2 for r in ratios)
    assert {c["C"] for c in AC.CASES} == {1, 3} and {c["size"][1] % 4 for c in AC.CASES} == {0, 1, 2, 3}
    assert any(c["size"] == (1, 1) for c in AC.CASES) and {7, 61} <= {c["size"][1] for c in AC.CASES}
    assert any(c["L"] == 2 and c.get("padded") and len(set(c["plans"])) == 2 for c in AC.CASES)
    assert any(AC.clamped(p, c["H0"], c["W0"]) != tuple(p) for c in AC.CASES for p in c["plans"])      # leaves the frame
    assert sum(c["size"][0] > 32 and c["size"][1] > 128 for c in AC.CASES) >= 1                          # 3 x 3 tiles
    assert sum(c["size"][0] > 16 and c["size"][1] > 64 and c["H0"] == 4 * c["size"][0] for c in AC.CASES) >= 1
    flips = {p[4] for c in AC.CASES for p in c["plans"]}
    assert flips == {0, 1}
    for h0, w0, (H, W) in AC.PAST_LIMIT:
        assert (h0 > AC.MAX_RATIO * H) != (w0 > AC.MAX_RATIO * W)
    assert set(AC.LIMITS) == set(IDS) and set(AC.PHOTO_LIMITS) == set(PC.ROWS)


# ---- the recorded limits, measured again -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", AC.CASES, ids=IDS)
def test_recorded_limit_is_three_times_the_float32_distance(case):
    _check_recorded(AC.LIMITS[case["name"]], measure(case), case["name"])


@pytest.mark.parametrize("name", list(PC.ROWS))
def test_recorded_photo_limit_is_three_times_the_float32_distance(name):
    _check_recorded(AC.PHOTO_LIMITS[name], measure_photo(name), name)


def test_recorded_end_to_end_limit_is_three_times_the_float32_distance():
    _check_recorded(AC.E2E_LIMIT, measure_e2e(), "end to end")


# ---- ABI, binding, refusals before any launch ---------------------------------------------------------------------------
def test_prototype_is_read_from_the_second_header():
    assert abi.EXT_PROTOTYPES[ENTRY] == (I, [P, P, I, I, I, I, I, I, I, LONG, LONG, P, P, P, P, P])
    assert abi.EXT_PROTOTYPES[ENTRY] == abi.EXT_PROTOTYPES["fod_clip_crop_resize_photo"]
    assert ENTRY not in abi.PROTOTYPES and ENTRY not in open(abi.HEADER_PATH).read()
    from future_od.native import lib as L
    assert ENTRY in L.EXT_SIGNATURES and ENTRY not in L.SIGNATURES and L.ABI_VERSION >= 16
    fn = getattr(L.LIB, ENTRY)
    assert fn.restype is abi.CTYPE[I] and list(fn.argtypes) == [abi.CTYPE[k] for k in abi.EXT_PROTOTYPES[ENTRY][1]]


def test_arguments_are_refused_before_any_launch():
    """The non-null 'pointers' are the address 1: a launch would fault, so a clean non-zero return is the check itself."""
    from future_od.native import lib as L
    fn, ERR_ARG = getattr(L.LIB, ENTRY), abi.CONSTANTS["FOD_ERR_ARG"]
    with pytest.raises(L.FodError, match="clip_crop_resize_aa"):
        L.call(ENTRY, None, None, 1, 1, 3, 8, 8, 4, 4, 192, 192, None, None, None, None, None)
    good = dict(src=1, dst=16, plans=1, mean=1, std=1)
    for missing in good:                                                  # each pointer in turn; photo may be NULL
        a = {**good, missing: None}
        rc = fn(a["src"], a["dst"], 1, 1, 3, 8, 8, 4, 4, 192, 192, a["plans"], a["mean"], a["std"], None, None)
        assert rc == ERR_ARG and "clip_crop_resize_aa" in L.last_error() and "null" in L.last_error(), missing
    for c in (1, 2):                                                      # photo rows need three planes
        assert fn(1, 16, 1, 1, c, 8, 8, 4, 4, 64 * c, 64 * c, 1, 1, 1, 1, None) == ERR_ARG and "three planes" in L.last_error()
    for c in (0, 4):
        assert fn(1, 16, 1, 1, c, 8, 8, 4, 4, 256, 256, 1, 1, 1, None, None) == ERR_ARG
    for bad in ((0, 1, 3, 8, 8, 4, 4, 192, 192), (1, 1, 3, 8, 8, 0, 4, 192, 192), (1, 1, 3, 8, 8, 4, 4, 100, 192),
                (1, 1, 3, 0, 8, 4, 4, 192, 192)):
        assert fn(1, 16, *bad, 1, 1, 1, None, None) == ERR_ARG, bad
    assert fn(1, 8, 1, 1, 3, 8, 8, 4, 4, 192, 192, 1, 1, 1, None, None) == ERR_ARG and "aligned" in L.last_error()
    # the ratio: decided from (H0, W0, H, W) alone -- one step past 4 on either axis
    for h0, w0, (H, W) in AC.PAST_LIMIT + [(17, 8, (4, 4)), (8, 17, (4, 4)), (900, 1600, (224, 400))]:
        n = 3 * h0 * w0
        assert fn(1, 16, 1, 1, 3, h0, w0, H, W, n, n, 1, 1, 1, None, None) == ERR_ARG, (h0, w0, H, W)
        assert "4 times" in L.last_error()


def test_wrapper_has_no_cpu_fallback():
    from future_od.native import lib as L
    from future_od.native import ops
    with pytest.raises(L.FodError, match="no CPU fallback"):
        ops.clip_crop_resize_aa(torch.zeros(1, 1, 3, 8, 8, dtype=torch.uint8), torch.zeros(1, 5, dtype=torch.int32),
                                (4, 4), torch.zeros(3), torch.ones(3))
    assert inspect.signature(ops.clip_crop_resize_aa).parameters["photo"].default is None


# ---- JointResize on the CPU ----------------------------------------------------------------------------------------------
def test_joint_resize_antialiases_on_the_cpu():
    import future_od.datasets.transforms as T
    g = torch.Generator().manual_seed(8)
    clip = torch.rand(2, 3, 50, 90, generator=g)
    boxes, classes = torch.tensor([[5.0, 6.0, 40.0, 30.0]]), torch.tensor([2])
    images, bx, cl = T.JointResize((24, 44), antialias=True)(clip, boxes, classes)
    assert torch.equal(images, F.interpolate(clip, size=(24, 44), mode="bilinear", align_corners=False, antialias=True))
    plain, bx0, cl0 = T.JointResize((24, 44))(clip, boxes, classes)
    assert torch.equal(plain, F.interpolate(clip, size=(24, 44), mode="bilinear", align_corners=False))
    assert not torch.equal(images, plain) and torch.equal(bx, bx0) and torch.equal(cl, cl0)
    assert inspect.signature(T.JointResize).parameters["antialias"].default is False
    for mode in ("nearest", "bicubic"):
        T.JointResize((24, 44), interpolation=mode)
        with pytest.raises(ValueError, match="antialias"):
            T.JointResize((24, 44), interpolation=mode, antialias=True)


def test_plans_boxes_and_draws_do_not_notice_the_flag():
    import future_od.datasets.transforms as T
    boxes = torch.tensor([[5.0, 6.0, 40.0, 30.0], [50.0, 20.0, 90.0, 55.0], [0.0, 0.0, 8.0, 8.0]])
    classes = torch.tensor([1, 2, 3])
    photo = T.JointPhotometricDistortion(p=0.8)
    assert T.Plan(8, 8).antialias is False
    for s in range(8):
        plans, states = [], []
        for flag in (False, True):
            rng = random.Random(s)
            t = T.JointCompose([T.RandomSizedCrop(0.5, 0.9), T.JointResize((32, 48), antialias=flag),
                                T.JointHorizontalFlip(0.5), T.SizeFilter(0.01), photo])
            plans.append(t.plan(60, 100, rng))
            states.append(rng.getstate())
        off, on = plans
        assert (off.antialias, on.antialias) == (False, True) and states[0] == states[1]
        assert off.row() == on.row() and off.size == on.size and off.steps == on.steps and repr(off) == repr(on)
        assert off.photo_row() == on.photo_row() and off.box_map() == on.box_map()
        (b0, c0), (b1, c1) = off.annotate(boxes, classes), on.annotate(boxes, classes)
        assert torch.equal(b0, b1) and torch.equal(c0, c1)
    # a plan without a resize does not antialias
    assert T.JointCompose([T.JointCenterCrop((30, 50))]).plan(60, 100, random.Random(0)).antialias is False


def test_uses_antialias_and_its_refusals():
    import future_od.datasets.transforms as T
    on, off = T.JointResize((32, 48), antialias=True), T.JointResize((32, 48))
    crop = T.RandomSizedCrop(0.5, 1.0)
    assert T.uses_antialias(on) and not T.uses_antialias(off) and not T.uses_antialias(crop)
    assert T.uses_antialias(T.JointCompose([crop, on, T.JointHorizontalFlip()]))
    assert not T.uses_antialias(T.JointCompose([crop, off])) and not T.uses_antialias(T.JointCompose([crop]))
    assert T.uses_antialias(T.RandomSelect(T.JointCompose([crop, on]), T.JointResize((32, 48), antialias=True)))
    assert T.uses_antialias(T.RandomSelect(on, T.JointCenterCrop((32, 48))))         # the other branch resamples nothing
    assert not T.uses_antialias(T.JointCompose([T.RandomSelect(off, T.JointNoOpTransform())]))
    for mixed in (T.RandomSelect(on, off), T.JointCompose([crop, T.RandomSelect(T.JointCompose([off]), on)]),
                  T.RandomSelect(T.JointCompose([crop, on]), T.JointCompose([T.JointCenterCrop((40, 60)), off]))):
        with pytest.raises(ValueError, match="antialias"):
            T.uses_antialias(mixed)
        from future_od.utils.augment import DeviceJointTransform
        with pytest.raises(ValueError, match="antialias"):
            DeviceJointTransform(mixed)


def test_host_half_is_the_same_with_and_without_the_flag():
    from future_od.utils.augment import DeviceJointTransform
    batch = e2e_batch()
    on, off = (DeviceJointTransform(e2e_transform(flag), seed=AC.E2E["seed"]) for flag in (True, False))
    assert on.antialias is True and off.antialias is False
    for index in range(3):
        a, b = on.host(batch), off.host(batch)
        assert set(a) == set(b) and a["_plan_size"] == b["_plan_size"] == AC.E2E["size"]
        for k in ("plans", "boxes", "classes", "active"):
            assert torch.equal(a[k], b[k]), k
    free = {k: v for k, v in batch.items() if k not in ("boxes", "classes", "active")}
    a, b = on.host(free, index=0), off.host(free, index=0)
    assert set(a) == set(b) and torch.equal(a["box_map"], b["box_map"]) and torch.equal(a["plans"], b["plans"])
    # the per-sample CPU transform draws what the host half draws: its boxes are the batch's
    out = on.host(batch, index=0)
    for b_, (_, boxes, classes, _) in enumerate(e2e_cpu(on, batch)):
        n = boxes.shape[0]
        assert int(out["active"][b_].sum()) == n and torch.equal(out["boxes"][b_, :n], boxes.to(out["boxes"].dtype))
        assert torch.equal(out["classes"][b_, :n], classes)
    with pytest.raises(RuntimeError, match="not on a GPU"):
        on.device(out)


# ---- loader keyword ----------------------------------------------------------------------------------------------------
def test_loaders_take_the_antialias_keyword():
    import future_od.datasets.transforms as T
    from runs._loader import get_nuim_loaders, get_nusc_loaders
    args, aug = SimpleNamespace(distributed=False), T.RandomSizedCrop(0.5, 1.0)
    for factory in (get_nusc_loaders, get_nuim_loaders):
        assert inspect.signature(factory).parameters["antialias"].default is False
        for photo in (None, T.JointPhotometricDistortion()):
            train, val = factory((32, 48), offsets=[-0.5, 0], config={}, args=args, train_batch_size=2, random_aug=aug,
                                 steps_per_epoch=2, val_steps=1, raw_size=(45, 80), antialias=True, photometric=photo)
            steps = train.device_transform.joint_transform.transforms
            assert len(steps) == 2 + (photo is not None) and steps[0] is aug and isinstance(steps[1], T.JointResize)
            assert steps[1]._antialias is True and steps[1]._size == [32, 48] and train.device_transform.antialias
            assert train.device_transform.photometric == (photo is not None)
            assert not val["val"].device_transform.antialias
        with pytest.raises(ValueError, match="random_aug"):
            factory((32, 48), offsets=[0], config={}, args=args, train_batch_size=2, antialias=True)
        with pytest.raises(TypeError, match="antialias"):                  # a step that lands on the flag is not a flag
            factory((32, 48), offsets=[0], config={}, args=args, train_batch_size=2, random_aug=aug, raw_size=(45, 80),
                    antialias=T.JointPhotometricDistortion())
        train, _ = factory((32, 48), offsets=[0], config={}, args=args, train_batch_size=2, random_aug=aug,
                           raw_size=(45, 80))
        assert train.device_transform.joint_transform.transforms[1]._antialias is False
        assert not train.device_transform.antialias


def test_run_script_has_the_flag():
    from runs.nusc_spatiotemporal_imu_500ms import build_parser
    assert build_parser().parse_args(["--antialias"]).antialias is True
    assert build_parser().parse_args([]).antialias is False


def test_measured_distances_are_rounding_noise():
    """Sanity of the yardstick itself: no recorded limit is above 1e-3 (normalised units span about +-2.6)."""
    for v in list(AC.LIMITS.values()) + list(AC.PHOTO_LIMITS.values()) + [AC.E2E_LIMIT]:
        assert math.isfinite(v) and 0 < v < 1e-3, v
