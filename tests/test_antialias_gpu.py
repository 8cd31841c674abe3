"""fod_clip_crop_resize_aa on the device: every output element of every case of tests/antialias_cases.py against the
float64 restatement under the case's recorded limit, the exact anchors (white frame, unchanged size), photometric rows,
the ratio refusal, and DeviceJointTransform end to end with the flag on and off."""
import pytest
import torch

import antialias_cases as AC
import photometric_cases as PC
from test_antialias_cpu import e2e_batch, e2e_cpu, e2e_transform

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -777.0
NAN, INF = float("nan"), float("inf")
IDS = [c["name"] for c in AC.CASES]


def _norm(C):
    return AC.MEAN[:C].contiguous().to(DEV), AC.STD[:C].contiguous().to(DEV)


def _raw_call(dev_u8, plans, size, photo=None):
    """The entry point itself, into a sentinel-filled destination -> (return code, destination)."""
    from future_od.native import lib as L
    from future_od.native.ops import ptr, stream
    B, Ln, C, H0, W0 = dev_u8.shape
    sb, sl = dev_u8.stride()[:2]
    mean, std = _norm(C)
    plans = torch.tensor(plans, dtype=torch.int32, device=DEV)
    dst = torch.full((B, Ln, C, *size), SENTINEL, dtype=torch.float32, device=DEV)
    rc = getattr(L.LIB, "fod_clip_crop_resize_aa")(ptr(dev_u8), ptr(dst), B, Ln, C, H0, W0, size[0], size[1], sb, sl,
                                                   ptr(plans), ptr(mean), ptr(std),
                                                   None if photo is None else ptr(photo), stream())
    torch.cuda.synchronize()
    return rc, dst


def _rows(rows):
    return torch.tensor(rows, dtype=torch.float32, device=DEV)


def _run(case, photo=None):
    dev = AC.view(AC.source(case).to(DEV), case)
    rc, dst = _raw_call(dev, case["plans"], case["size"], photo)
    assert rc == 0
    return dev, dst


# ---- a. every case, every element ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", AC.CASES, ids=IDS)
def test_every_output_element_against_float64(case):
    dev, dst = _run(case)
    got = dst.cpu()
    assert not bool((got == SENTINEL).any()) and bool(torch.isfinite(got).all())        # every element was written
    want = AC.expected(case, dev.cpu(), torch.float64)
    assert got.shape == want.shape
    dist, limit = float((got.double() - want).abs().max()), AC.LIMITS[case["name"]]
    print(f"\n{case['name']}: kernel to f64 max {dist:.3e}, limit {limit:.3e}")
    assert dist <= limit, (dist, limit)
    if case["kind"] == "white":
        flat = ((1 - AC.MEAN.double()) / AC.STD.double()).view(1, 1, 3, 1, 1)
        assert float((got.double() - flat).abs().max()) <= limit
    if case["kind"] == "pixel":
        assert float(got.max()) > float(got.min())                                       # the pixel is in the picture
    if case.get("unchanged"):
        from future_od.native import ops
        plans = torch.tensor(case["plans"], dtype=torch.int32, device=DEV)
        assert torch.equal(dst, ops.clip_crop_resize(dev, plans, case["size"], *_norm(case["C"])))
    # the wrapper gives the same bits
    from future_od.native import ops
    out = ops.clip_crop_resize_aa(dev, torch.tensor(case["plans"], dtype=torch.int32, device=DEV), case["size"],
                                  *_norm(case["C"]))
    assert torch.equal(out, dst)


def test_antialiasing_reads_what_two_taps_skip():
    """Columns in the pattern 0 0 255 255, reduced 3 : 1.  The two-tap pass samples source column 3 o + 2 with weight 1
    (s = 3 (o + 0.5) - 0.5 is a whole number): every output is 0 or 1, the pattern aliases.  The footprint filter, a
    triangle of half-width 3 over a period of 4, leaves about 0.06 of the swing around the mean 0.5."""
    from future_od.native import ops
    u8 = torch.zeros(1, 1, 3, 32, 128, dtype=torch.uint8)
    u8[..., 2::4] = 255
    u8[..., 3::4] = 255
    plans = torch.tensor([(0, 1, 32, 126, 0)], dtype=torch.int32, device=DEV)
    mean, std = torch.zeros(3, device=DEV), torch.ones(3, device=DEV)
    aa = ops.clip_crop_resize_aa(u8.to(DEV), plans, (16, 42), mean, std)[..., 2:-2]
    two = ops.clip_crop_resize(u8.to(DEV), plans, (16, 42), mean, std)[..., 2:-2]
    assert float((aa - 0.5).abs().max()) < 0.2 < float((two - 0.5).abs().max())


# ---- b. photometric rows ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PC.ROWS))
def test_photo_rows_against_float64(name):
    case = AC.PHOTO_CASE
    dev, dst = _run(case, _rows([PC.ROWS[name]] * case["B"]))
    got = dst.cpu()
    assert not bool((got == SENTINEL).any()) and bool(torch.isfinite(got).all())
    want = AC.expected(case, dev.cpu(), None, lambda crop, size: PC.normalise(
        PC.restated(AC.sample(crop, size, torch.float64) / 255, PC.ROWS[name], torch.float64)))
    dist, limit = float((got.double() - want).abs().max()), AC.PHOTO_LIMITS[name]
    print(f"\n{name}: kernel to f64 max {dist:.3e}, limit {limit:.3e}")
    assert dist <= limit, (dist, limit)


def test_neutral_rows_nan_rows_and_one_row_per_clip():
    from future_od.native import ops
    case = AC.PHOTO_CASE
    dev, plain = _run(case)
    for rows in ([PC.NEUTRAL, (0.0, 1.0, 1.0, 0.0, 1.0)], [(NAN, INF, -INF, NAN, NAN), (0.0, 1.0, 1.0, -7.0, 3.0)]):
        assert torch.equal(_run(case, _rows(rows))[1], plain), rows                      # the bits of photo = NULL
    wild = _run(case, _rows([(NAN,) * 5, (0.05, NAN, 1e30, -INF, NAN)]))[1]
    tame = _run(case, _rows([(0.0, 1.0, 1.0, 0.0, 1.0), (0.05, 1.0, 4.0, 0.0, 1.0)]))[1]
    assert bool(torch.isfinite(wild).all()) and torch.equal(wild, tame)
    assert torch.equal(wild[0], plain[0]) and not torch.equal(wild[1], plain[1])
    # one row per clip, through the wrapper: clip 0 neutral, clip 1 active
    plans = torch.tensor(case["plans"], dtype=torch.int32, device=DEV)
    mixed = ops.clip_crop_resize_aa(dev, plans, case["size"], *_norm(3), _rows([PC.NEUTRAL, PC.ROWS["hue"]]))
    hue = _run(case, _rows([PC.ROWS["hue"]] * 2))[1]
    assert torch.equal(mixed[0], plain[0]) and torch.equal(mixed[1], hue[1])


# ---- c. refusals --------------------------------------------------------------------------------------------------------
def test_ratio_past_the_limit_is_refused_and_nothing_is_written():
    from future_od.native import abi
    from future_od.native import lib as L
    from future_od.native import ops
    for h0, w0, size in AC.PAST_LIMIT:
        dev = torch.zeros(1, 1, 3, h0, w0, dtype=torch.uint8, device=DEV)
        plan = [(0, 0, 4, 4, 0)]                          # the rectangle is tiny: the plan's contents decide nothing
        rc, dst = _raw_call(dev, plan, size)
        assert rc == abi.CONSTANTS["FOD_ERR_ARG"] and "4 times" in L.last_error()
        assert bool((dst == SENTINEL).all())
        with pytest.raises(L.FodError, match="4 times"):
            ops.clip_crop_resize_aa(dev, torch.tensor(plan, dtype=torch.int32, device=DEV), size, *_norm(3))
    u8 = torch.zeros(2, 1, 3, 8, 12, dtype=torch.uint8, device=DEV)
    plans = torch.zeros(2, 5, dtype=torch.int32, device=DEV)
    mean, std = _norm(3)
    photo = _rows([PC.NEUTRAL] * 2)
    assert ops.clip_crop_resize_aa(u8, plans, (4, 4), mean, std, photo).shape == (2, 1, 3, 4, 4)
    for bad in (lambda: ops.clip_crop_resize_aa(u8, plans, (4, 4), mean, std, photo.double()),
                lambda: ops.clip_crop_resize_aa(u8, plans, (4, 4), mean, std, photo[:1]),
                lambda: ops.clip_crop_resize_aa(u8, plans, (4, 4), mean, std, photo.cpu()),
                lambda: ops.clip_crop_resize_aa(u8[:, :, :1].contiguous(), plans, (4, 4), mean[:1].contiguous(),
                                                std[:1].contiguous(), photo),
                lambda: ops.clip_crop_resize_aa(u8.float(), plans, (4, 4), mean, std),
                lambda: ops.clip_crop_resize_aa(u8, plans[:1], (4, 4), mean, std),
                lambda: ops.clip_crop_resize_aa(u8, plans, (0, 4), mean, std)):
        with pytest.raises(L.FodError):
            bad()


# ---- d. end to end ------------------------------------------------------------------------------------------------------
def _to_device(batch):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}


def test_device_transform_end_to_end_with_the_flag_on_and_off():
    import future_od.datasets.transforms as T
    from future_od.native import ops
    from future_od.utils.augment import DeviceJointTransform
    batch, size, seed = e2e_batch(), AC.E2E["size"], AC.E2E["seed"]
    mean, std = _norm(3)
    on, off = (DeviceJointTransform(e2e_transform(flag), seed=seed) for flag in (True, False))
    host_on, host_off = on.host(batch, index=0), off.host(batch, index=0)
    got = on.device(_to_device(host_on))
    torch.cuda.synchronize()
    assert set(got) == set(batch) and got["video"].shape == (AC.E2E["B"], AC.E2E["L"], 3, *size)
    for b, (images, boxes, classes, exact) in enumerate(e2e_cpu(on, batch)):
        video = got["video"][b].cpu().double()
        assert float((video - exact).abs().max()) <= AC.E2E_LIMIT                        # the kernel ...
        assert float((images.double() - exact).abs().max()) <= AC.E2E_LIMIT              # ... and the CPU transform
        apart = float((video - images.double()).abs().max())                             # ... and the two, directly
        print(f"\nsample {b}: kernel to the per-sample CPU transform max {apart:.3e}, limit {AC.E2E_LIMIT:.3e}")
        assert apart <= AC.E2E_LIMIT, (b, apart)
        n = boxes.shape[0]
        assert torch.equal(got["boxes"][b, :n].cpu(), boxes.to(got["boxes"].dtype))
    # off: today's launch, today's bits
    plain = off.device(_to_device(host_off))
    want = ops.clip_crop_resize(batch["video"].to(DEV), host_off["plans"].to(DEV), size, mean, std)
    assert torch.equal(plain["video"], want) and not torch.equal(plain["video"], got["video"])
    # on, with a photometric step: the rows go through the same launch
    photo = T.JointPhotometricDistortion(p=1.0)
    both = DeviceJointTransform(e2e_transform(True, photo), seed=seed)
    host = both.host(batch, index=0)
    assert torch.equal(host["plans"], host_on["plans"]) and host["photo"].shape == (AC.E2E["B"], 5)
    out = both.device(_to_device(host))
    assert set(out) == set(batch)
    want = ops.clip_crop_resize_aa(batch["video"].to(DEV), host["plans"].to(DEV), size, mean, std, host["photo"].to(DEV))
    assert torch.equal(out["video"], want) and not torch.equal(out["video"], got["video"])
    assert bool(torch.isfinite(out["video"]).all())
