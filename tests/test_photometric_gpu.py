"""fod_clip_crop_resize_photo on the device: neutral rows against fod_clip_crop_resize bit for bit, active rows against a
float64 evaluation of the definition (tests/photometric_cases.py) with the float32 CPU evaluation as the yardstick, one
row per clip, rows that must be sanitised, the wrapper's refusals, and the loaders' `photometric` step end to end
(DevicePrefetcher -> captured step)."""
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import photometric_cases as PC
from test_augment_gpu import CASES as PARENT_CASES
from test_augment_gpu import _build, _source_index

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN, STD = PC.MEAN, PC.STD
NAN, INF = float("nan"), float("inf")


def _photo(u8, plans, size, rows, dev_u8=None):
    from future_od.native import ops
    out = ops.clip_crop_resize_photo(u8.to(DEV) if dev_u8 is None else dev_u8,
                                     torch.tensor(plans, dtype=torch.int32, device=DEV), size, MEAN.to(DEV), STD.to(DEV),
                                     torch.tensor(rows, dtype=torch.float32, device=DEV))
    torch.cuda.synchronize()
    return out


def _parent(u8, plans, size, dev_u8=None):
    from future_od.native import ops
    out = ops.clip_crop_resize(u8.to(DEV) if dev_u8 is None else dev_u8,
                               torch.tensor(plans, dtype=torch.int32, device=DEV), size, MEAN.to(DEV), STD.to(DEV))
    torch.cuda.synchronize()
    return out


# ---- a. neutral rows: the parent kernel's bits ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", PARENT_CASES, ids=[c[0] for c in PARENT_CASES])
def test_neutral_rows_give_the_parent_kernels_bits(case):
    """The parent test's cases (W % 4 in {0, 3, 2}, W < 4, flips, per-sample rectangles, up- and down-scaling, and the
    2 x 6 x 900 x 1600 -> 896 x 1600 extent); both outputs stay on the device.  `first` is free in a neutral row, and a
    row that is neutral only once it is sanitised counts too."""
    name, B, L, H0, W0, size, plans = case
    g = torch.Generator().manual_seed(H0 * 7 + W0)
    dev_u8 = torch.randint(0, 256, (B, L, 3, H0, W0), generator=g, dtype=torch.uint8).to(DEV)
    neutral = [(0.0, 1.0, 1.0, 0.0, 0.0), (0.0, 1.0, 1.0, 0.0, 1.0), (NAN, INF, -INF, NAN, NAN), (0.0, 1.0, 1.0, -7.0, 3.0)]
    want = _parent(None, plans, size, dev_u8)
    for shift in range(2):
        rows = [neutral[(b + shift) % 4] for b in range(B)]
        got = _photo(None, plans, size, rows, dev_u8)
        assert got.shape == want.shape == (B, L, 3, *size) and got.dtype == torch.float32
        assert torch.equal(got, want), (name, rows)


# ---- b. parity against float64 -----------------------------------------------------------------------------------------
def _sample(crop_u8, size, dtype):
    """The bilinear sample of fod_clip_crop_resize (the parent test's gather) on one cropped clip [L, 3, h, w], divided by
    255 and NOT normalised, every step in `dtype`."""
    h, w = crop_u8.shape[-2:]
    H, W = size
    p = crop_u8.to(dtype)
    y0, y1, ly = _source_index(h / H, H, h, dtype)
    x0, x1, lx = _source_index(w / W, W, w, dtype)
    ly, lx = ly.view(H, 1), lx.view(1, W)
    top = (1 - lx) * p[..., y0, :][..., x0] + lx * p[..., y0, :][..., x1]
    bot = (1 - lx) * p[..., y1, :][..., x0] + lx * p[..., y1, :][..., x1]
    return ((1 - ly) * top + ly * bot) / 255


def _yardstick_f32(crop_u8, size, row):
    """The same chain as torch evaluates it in f32 on the CPU: its bilinear resize, / 255, the map, the normalisation."""
    p = F.interpolate(crop_u8.float(), size=size, mode="bilinear", align_corners=False) / 255
    return PC.normalise(PC.restated(p, row, torch.float32))


# (name, H0, W0, (H, W), plans, rows): B = 3, L = 2, at least 10 000 output pixels per frame, another row per sample.
# Together: every stage alone, all stages in both contrast orders, a neutral sample among active ones, W % 4 in
# {0, 1, 2, 3}, one flipped sample per case, up- and down-scaling.  The structured blocks of PC.structured_frames lie
# in the top rows of the source, inside the first sample's rectangle of every case.
# No rectangle is larger than 128 either way.  The f32 distance of the whole chain is not the map's (a few 1e-6,
# tests/test_photometric_cpu.py) but the source coordinate's: s = scale * (o + 0.5) - 0.5 carries half an ulp of s, that
# is 2^-18 = 3.8e-6 below 128, into the bilinear weight, where it meets a pixel step of up to 1 on noise, the row's gain
# (contrast 1.3 x saturation 1.4 x the hue ramp's slope, together up to 5 or so) and 1 / std = 4.4: up to 1e-4 normalised
# for the row with every stage and the contrast last, half of that for the others.  That row's upscaled sample therefore
# stays below 64, and above 128 everything doubles, which leaves the yardstick's sanity bound of 1e-4 no room.
PARITY = [
    ("W % 4 = 0: brightness, contrast, saturation alone", 110, 140, (100, 104),
     [(0, 0, 90, 128, 0), (5, 9, 100, 120, 1), (20, 30, 60, 90, 0)], ["brightness", "contrast", "saturation"]),
    ("W % 4 = 1: hue alone, all stages in both orders", 110, 140, (101, 101),
     [(0, 0, 110, 128, 0), (9, 20, 101, 101, 0), (3, 5, 105, 126, 1)],
     ["hue", "all, contrast after", "all, contrast first"]),
    ("W % 4 = 2: a neutral sample among active ones", 110, 140, (100, 102),
     [(0, 0, 75, 128, 1), (10, 12, 90, 120, 0), (0, 12, 60, 64, 0)], ["all, contrast first", None, "all, contrast after"]),
    ("W % 4 = 3: the stages alone, the other way", 110, 140, (98, 103),
     [(0, 0, 64, 128, 0), (7, 3, 100, 127, 1), (30, 40, 80, 100, 0)], ["desaturation", "hue back", "contrast down"]),
]
FACTOR = 2.0          # as the parent's test: both sides evaluate one f32 formula, apart in contraction and division rounding


@pytest.mark.parametrize("case", PARITY, ids=[c[0] for c in PARITY])
def test_kernel_against_float64(case):
    """Bound: the kernel's max and mean absolute distance to the f64 value at most FACTOR x the f32 CPU evaluation's own
    max and mean distance to it, in normalised units.  Measured ratios: profiles/photometric_kernel_rates.txt."""
    name, H0, W0, size, plans, names = case
    B, L = 3, 2
    assert size[0] * size[1] >= 10000 and len(plans) == len(names) == B
    u8 = torch.stack([PC.structured_frames(L, H0, W0, seed=H0 + 31 * b + size[1]) for b in range(B)])
    rows = [PC.NEUTRAL if n is None else PC.ROWS[n] for n in names]
    got = _photo(u8, plans, size, rows).cpu()
    assert got.shape == (B, L, 3, *size) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    k_max = r_max = k_sum = r_sum = 0.0
    for b, (top, left, h, w, flip) in enumerate(plans):
        crop = u8[b, :, :, top:top + h, left:left + w]
        exact = PC.normalise(PC.restated(_sample(crop, size, torch.float64), rows[b], torch.float64))
        ref = _yardstick_f32(crop, size, rows[b])
        if flip:
            exact, ref = exact.flip(-1), ref.flip(-1)
        dk, dr = (got[b].double() - exact).abs(), (ref.double() - exact).abs()
        k_max, r_max = max(k_max, float(dk.max())), max(r_max, float(dr.max()))
        k_sum, r_sum = k_sum + float(dk.sum()), r_sum + float(dr.sum())
    n = got.numel()
    print(f"\n{name}: kernel max {k_max:.3e} mean {k_sum / n:.3e} | f32 CPU max {r_max:.3e} mean {r_sum / n:.3e} | "
          f"ratios max {k_max / r_max:.2f} mean {k_sum / r_sum:.2f}")
    assert r_max < 1e-4, r_max                       # the yardstick itself is sane (normalised units span ~ +-2.6)
    assert k_max <= FACTOR * r_max, (k_max, r_max)
    assert k_sum / n <= FACTOR * r_sum / n, (k_sum / n, r_sum / n)


# ---- c. one row per clip -----------------------------------------------------------------------------------------------
def test_one_row_serves_every_frame_of_its_clip():
    frame = PC.structured_frames(1, 60, 90, seed=2)                                     # [1, 3, 60, 90]
    u8 = frame.expand(4, 3, 60, 90).unsqueeze(0).expand(2, 4, 3, 60, 90).contiguous()   # two clips of four copies
    plans = [(5, 10, 50, 70, 0)] * 2
    got = _photo(u8, plans, (44, 62), [PC.ROWS["all, contrast after"], PC.ROWS["all, contrast first"]])
    for b in range(2):
        for l in range(1, 4):
            assert torch.equal(got[b, l], got[b, 0]), (b, l)
    assert not torch.equal(got[0], got[1])
    assert float((got[0] - got[1]).abs().mean()) > 1e-2                                 # another row, another picture


# ---- d. rows that must be sanitised ------------------------------------------------------------------------------------
def test_wild_rows_are_sanitised():
    """NaN, +-inf, 1e30 and -7 in each field in turn.  What the kernel must make of them, written out: a non-finite
    number becomes the field's neutral value; then delta -> [-1, 1], alpha and sat -> [0, 4], hue -> hue - floor(hue);
    `first` counts as set unless it equals 0."""
    base = (0.05, 1.2, 1.3, 0.04, 0.0)
    wild_values = (NAN, INF, -INF, 1e30, -7.0)
    tame_values = [(0.0, 0.0, 0.0, 1.0, -1.0),       # delta
                   (1.0, 1.0, 1.0, 4.0, 0.0),        # alpha
                   (1.0, 1.0, 1.0, 4.0, 0.0),        # sat
                   (0.0, 0.0, 0.0, 0.0, 0.0),        # hue: 1e30 and -7 are whole numbers
                   (1.0, 1.0, 1.0, 1.0, 1.0)]        # first
    wild, tame = [], []
    for field in range(5):
        for w, t in zip(wild_values, tame_values[field]):
            wild.append(tuple(w if i == field else v for i, v in enumerate(base)))
            tame.append(tuple(t if i == field else v for i, v in enumerate(base)))
    wild += [(NAN,) * 5, (INF,) * 5, (-INF, 1e30, -1e30, 1e30, 0.0)]
    tame += [(0.0, 1.0, 1.0, 0.0, 1.0), (0.0, 1.0, 1.0, 0.0, 1.0), (0.0, 4.0, 0.0, 0.0, 0.0)]
    B = len(wild)
    u8 = PC.structured_frames(B, 24, 40, seed=9).unsqueeze(1)                           # [B, 1, 3, 24, 40]
    plans = [(2, 3, 20, 33, b % 2) for b in range(B)]
    got, want = _photo(u8, plans, (19, 27), wild), _photo(u8, plans, (19, 27), tame)
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, want)
    for b in range(B):                                                                  # and they are what the CPU form reads
        assert PC.sanitised(wild[b]) == PC.sanitised(tame[b]), wild[b]


# ---- e. wrapper refusals -----------------------------------------------------------------------------------------------
def test_wrapper_refuses_what_the_kernel_cannot_take():
    from future_od.native import lib as L
    from future_od.native import ops
    u8 = torch.zeros(2, 1, 3, 8, 12, dtype=torch.uint8, device=DEV)
    plans = torch.zeros(2, 5, dtype=torch.int32, device=DEV)
    photo = torch.tensor([PC.NEUTRAL] * 2, dtype=torch.float32, device=DEV)
    mean, std = MEAN.to(DEV), STD.to(DEV)
    assert ops.clip_crop_resize_photo(u8, plans, (4, 4), mean, std, photo).shape == (2, 1, 3, 4, 4)
    for bad in (lambda: ops.clip_crop_resize_photo(u8, plans, (4, 4), mean, std, photo.double()),
                lambda: ops.clip_crop_resize_photo(u8, plans, (4, 4), mean, std, photo[:1]),
                lambda: ops.clip_crop_resize_photo(u8, plans, (4, 4), mean, std, photo[:, :4].contiguous()),
                lambda: ops.clip_crop_resize_photo(u8, plans, (4, 4), mean, std, photo.flatten()),
                lambda: ops.clip_crop_resize_photo(u8, plans, (4, 4), mean, std, photo.cpu()),
                lambda: ops.clip_crop_resize_photo(u8, plans, (4, 4), mean, std, None),
                lambda: ops.clip_crop_resize_photo(u8, plans, (4, 4), mean, std, [PC.NEUTRAL] * 2),
                lambda: ops.clip_crop_resize_photo(u8[:, :, :2].contiguous(), plans, (4, 4), mean[:2].contiguous(),
                                                   std[:2].contiguous(), photo),
                lambda: ops.clip_crop_resize_photo(u8[..., ::2], plans, (4, 4), mean, std, photo),
                lambda: ops.clip_crop_resize_photo(u8.float(), plans, (4, 4), mean, std, photo),
                lambda: ops.clip_crop_resize_photo(u8, plans.long(), (4, 4), mean, std, photo),
                lambda: ops.clip_crop_resize_photo(u8, plans, (0, 4), mean, std, photo)):
        with pytest.raises(L.FodError):
            bad()


# ---- f. end to end -----------------------------------------------------------------------------------------------------
def test_photometric_loader_through_prefetcher_and_captured_step():
    import future_od.datasets.transforms as T
    from future_od.graph import GraphedStep
    from future_od.native import ops
    from future_od.utils.prefetch import DevicePrefetcher
    from runs._loader import get_nusc_loaders
    train, val = get_nusc_loaders((64, 96), offsets=[-1.0, -0.5, 0], config={}, args=SimpleNamespace(distributed=False),
                                  train_batch_size=2, random_aug=T.RandomSizedCrop(0.5, 1.0), steps_per_epoch=4,
                                  val_steps=1, raw_size=(90, 160), photometric=T.JointPhotometricDistortion(p=0.8))
    dt = train.device_transform
    planned, host_half = [], dt.host

    def recording_host(batch, index=None):
        out = host_half(batch, index)
        planned.append((out["plans"].clone(), out["photo"].clone()))
        return out

    dt.host = recording_host
    raw = list(train)
    got = list(DevicePrefetcher(train, DEV))
    torch.cuda.synchronize()
    assert len(got) == len(planned) == 4
    mean, std = MEAN.to(DEV), STD.to(DEV)
    for src, (plans, photo), b in zip(raw, planned, got):
        assert set(b) == set(src) and "plans" not in b and "photo" not in b          # exactly the source's keys
        assert b["video"].is_cuda and b["video"].dtype == torch.float32 and b["video"].shape == (2, 3, 3, 64, 96)
        assert photo.shape == (2, 5) and photo.dtype == torch.float32
        want = ops.clip_crop_resize_photo(src["video"].to(DEV), plans.to(DEV), (64, 96), mean, std, photo.to(DEV))
        assert torch.equal(b["video"], want)
        plain = ops.clip_crop_resize(src["video"].to(DEV), plans.to(DEV), (64, 96), mean, std)
        assert not torch.equal(b["video"], plain)                                     # the rows did something
    assert all(not torch.equal(p[1], q[1]) for p, q in zip(planned, planned[1:]))     # consecutive batches, other rows
    assert len({tuple(p[1].flatten().tolist()) for p in planned}) == 4
    # the validation loader has no photometric step
    (vb,), (vraw,) = list(DevicePrefetcher(val["val"], DEV)), list(val["val"])
    assert set(vb) == set(vraw) and not val["val"].device_transform.photometric

    # a few captured steps: ONE capture, finite losses
    model, opt = _build()
    step = GraphedStep(model, opt, warmup=2)
    losses = [float(step(b)[1].detach()) for b in DevicePrefetcher(train, DEV)]
    assert step.replays == 4 and len(step._graphs) == 1
    assert all(l == l and abs(l) < 1e6 for l in losses), losses
    assert len(planned) == 8 and not torch.equal(planned[4][1], planned[0][1])        # the second epoch draws anew
