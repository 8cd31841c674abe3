"""Device half of the joint crop / resize augmentation: fod_clip_crop_resize against torch, its exact cases, and the
augmenting loaders end to end (DevicePrefetcher -> captured step -> Trainer)."""
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEAN, STD = torch.tensor([0.485, 0.456, 0.406]), torch.tensor([0.229, 0.224, 0.225])


def _norm(v, dtype):
    return ((v / 255) - MEAN.to(dtype).view(1, 3, 1, 1)) / STD.to(dtype).view(1, 3, 1, 1)


def _source_index(scale, n_out, extent, dtype):
    s = (scale * (torch.arange(n_out, dtype=dtype) + 0.5) - 0.5).clamp(min=0)
    i0 = s.floor().clamp(max=extent - 1)
    i1 = (i0 + 1).clamp(max=extent - 1)
    return i0.long(), i1.long(), s - i0


def _gather_f64(crop_u8, size):
    """The formula of fod_clip_crop_resize on one cropped clip [L, 3, h, w], every step in f64: the exact value."""
    h, w = crop_u8.shape[-2:]
    H, W = size
    p = crop_u8.double()
    y0, y1, ly = _source_index(h / H, H, h, torch.float64)
    x0, x1, lx = _source_index(w / W, W, w, torch.float64)
    ly, lx = ly.view(H, 1), lx.view(1, W)
    top = (1 - lx) * p[..., y0, :][..., x0] + lx * p[..., y0, :][..., x1]
    bot = (1 - lx) * p[..., y1, :][..., x0] + lx * p[..., y1, :][..., x1]
    return _norm((1 - ly) * top + ly * bot, torch.float64)


def _reference_f32(crop_u8, size):
    """The same formula as torch evaluates it in f32 on the CPU (the reference's resize arithmetic)."""
    return _norm(F.interpolate(crop_u8.float(), size=size, mode="bilinear", align_corners=False), torch.float32)


def _kernel(u8, plans, size):
    from future_od.native import ops
    out = ops.clip_crop_resize(u8.to(DEV), torch.tensor(plans, dtype=torch.int32, device=DEV), size, MEAN.to(DEV),
                               STD.to(DEV))
    torch.cuda.synchronize()
    return out.cpu()


# (name, B, L, H0, W0, (H, W), plans); the rectangles stay inside the frame.  Every case has about a thousand outputs or
# more: both distances are rounding noise of a few ulp on small frames, and a ratio of two maxima over a handful of
# values would measure luck.
CASES = [
    ("upscale, per-sample plans, flip, bottom/right edges", 3, 2, 45, 80, (64, 96),
     [(0, 0, 30, 50, 0), (15, 30, 30, 50, 1), (5, 7, 23, 41, 0)]),
    ("downscale, odd sizes, W % 4 = 3, top/left edges", 3, 2, 45, 80, (17, 27),
     [(0, 0, 45, 80, 0), (0, 29, 45, 51, 1), (12, 0, 33, 80, 0)]),
    ("W % 4 = 2, single frame, mixed up/down", 2, 1, 33, 47, (40, 30), [(3, 5, 29, 41, 1), (0, 0, 33, 47, 0)]),
    ("W < 4", 1, 3, 30, 11, (37, 3), [(4, 3, 20, 5, 0)]),
    ("real extent, stage 2", 2, 6, 900, 1600, (896, 1600), [(0, 0, 900, 1600, 0), (131, 207, 620, 1103, 1)]),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_kernel_against_torch(case):
    """Bound (set with the kernel): max and mean absolute distance to the f64 value at most 2 x the f32 torch
    evaluation's own max and mean distance to it, on uint8 noise frames."""
    name, B, L, H0, W0, size, plans = case
    g = torch.Generator().manual_seed(H0 * 7 + W0)
    u8 = torch.randint(0, 256, (B, L, 3, H0, W0), generator=g, dtype=torch.uint8)
    got = _kernel(u8, plans, size)
    assert got.shape == (B, L, 3, *size) and got.dtype == torch.float32
    k_max = r_max = k_sum = r_sum = 0.0
    for b, (top, left, h, w, flip) in enumerate(plans):
        crop = u8[b, :, :, top:top + h, left:left + w]
        exact, ref = _gather_f64(crop, size), _reference_f32(crop, size)
        if flip:
            exact, ref = exact.flip(-1), ref.flip(-1)
        dk, dr = (got[b].double() - exact).abs(), (ref.double() - exact).abs()
        k_max, r_max = max(k_max, float(dk.max())), max(r_max, float(dr.max()))
        k_sum, r_sum = k_sum + float(dk.sum()), r_sum + float(dr.sum())
    n = got.numel()
    print(f"\n{name}: kernel max {k_max:.3e} mean {k_sum / n:.3e} | f32 torch max {r_max:.3e} mean {r_sum / n:.3e}")
    assert r_max < 1e-3, r_max                       # the yardstick itself is sane (normalised units span ~ +-2.6)
    assert k_max <= 2 * r_max, (k_max, r_max)
    assert k_sum / n <= 2 * r_sum / n, (k_sum / n, r_sum / n)


def test_rectangle_that_leaves_the_frame_is_clamped_into_it():
    """The kernel reads the plans from device memory; whatever they hold, it samples inside the frame: the extent is
    clamped first, then the origin."""
    g = torch.Generator().manual_seed(3)
    u8 = torch.randint(0, 256, (4, 2, 3, 45, 80), generator=g, dtype=torch.uint8)
    wild = [(-5, 70, 30, 50, 0), (40, -9, 30, 50, 1), (7, 11, 4000, -3, 0), (2 ** 30, 2 ** 30, 2 ** 30, 2 ** 30, 0)]
    tame = [(0, 30, 30, 50, 0), (15, 0, 30, 50, 1), (0, 11, 45, 1, 0), (0, 0, 45, 80, 0)]
    assert torch.equal(_kernel(u8, wild, (24, 36)), _kernel(u8, tame, (24, 36)))


def test_exact_where_exactness_exists():
    from future_od.native import ops
    g = torch.Generator().manual_seed(11)
    u8 = torch.randint(0, 256, (2, 3, 3, 45, 80), generator=g, dtype=torch.uint8)
    # the validation centre crop: height == H, width == W copies the rectangle
    got = _kernel(u8, [(6, 16, 32, 48, 0), (13, 32, 32, 48, 0)], (32, 48))
    for b, (top, left) in enumerate([(6, 16), (13, 32)]):
        want = _norm(u8[b, :, :, top:top + 32, left:left + 48].float(), torch.float32)
        assert torch.equal(got[b], want)
    flipped = _kernel(u8, [(6, 16, 32, 48, 1), (13, 32, 32, 48, 1)], (32, 48))
    assert torch.equal(flipped, got.flip(-1))
    # an identity plan is indistinguishable from the uint8 ingest of the stem
    ident = torch.tensor([(0, 0, 45, 80, 0)] * 2, dtype=torch.int32, device=DEV)
    mean, std, dev_u8 = MEAN.to(DEV), STD.to(DEV), u8.to(DEV)
    video = ops.clip_crop_resize(dev_u8, ident, (45, 80), mean, std)
    for dtype in (torch.bfloat16, torch.float32):
        a = ops.clip_to_stem_layout(video, dtype)
        b = ops.clip_to_stem_layout(dev_u8, dtype, mean, std)
        assert a.shape == b.shape and torch.equal(a, b), dtype
    # a strided source: the frames of a [L, B] upload viewed as [B, L]
    lb = u8.transpose(0, 1).contiguous().to(DEV)
    again = ops.clip_crop_resize(lb.transpose(0, 1), ident, (45, 80), mean, std)
    assert torch.equal(again, video)


def test_wrapper_refuses_what_the_kernel_cannot_take():
    from future_od.native import lib as L
    from future_od.native import ops
    u8 = torch.zeros(2, 1, 3, 8, 12, dtype=torch.uint8, device=DEV)
    plans = torch.zeros(2, 5, dtype=torch.int32, device=DEV)
    mean, std = MEAN.to(DEV), STD.to(DEV)
    for bad in (lambda: ops.clip_crop_resize(u8.float(), plans, (4, 4), mean, std),
                lambda: ops.clip_crop_resize(u8, plans.long(), (4, 4), mean, std),
                lambda: ops.clip_crop_resize(u8, plans[:1], (4, 4), mean, std),
                lambda: ops.clip_crop_resize(u8, plans.cpu(), (4, 4), mean, std),
                lambda: ops.clip_crop_resize(u8[..., ::2], plans, (4, 4), mean, std),
                lambda: ops.clip_crop_resize(u8, plans, (0, 4), mean, std)):
        with pytest.raises(L.FodError):
            bad()


def _build(dtype="bf16", seed=3):
    from future_od.models.st_detr import SpatioTemporalDETRArgs
    from future_od.optim import FusedAdamW
    from oracle import stdetr as O
    from runs._model import build_model
    cfg = O.Config(backbone="resnet18", enc_layers=1, dec_layers=2)
    args = SimpleNamespace(device=DEV, distributed=False, compute_dtype=dtype, backbone="resnet18")
    detr = SpatioTemporalDETRArgs(num_classes=8, num_queries=128, lr_backbone=1e-4, enc_layers=1, dec_layers=2,
                                  pretrained_backbone=False)
    model = build_model(args, detr)
    model.load_state_dict(O.make_state_dict(cfg, seed))
    model.eval()
    return model, FusedAdamW(model.parameters(), lr=1e-4, weight_decay=1e-4, max_norm=0.1)


def _aug_loaders(steps, val_steps=1):
    import future_od.datasets.transforms as T
    from runs._loader import get_nusc_loaders
    return get_nusc_loaders((64, 96), offsets=[-1.0, -0.5, 0], config={}, args=SimpleNamespace(distributed=False),
                            train_batch_size=2, random_aug=T.RandomSizedCrop(0.5, 1.0), steps_per_epoch=steps,
                            val_steps=val_steps, raw_size=(90, 160))


def test_augmenting_loader_through_prefetcher_and_captured_step():
    from future_od.graph import GraphedStep
    from future_od.native import ops
    from future_od.utils.prefetch import DevicePrefetcher
    train, val = _aug_loaders(steps=4)
    dt = train.device_transform
    planned, host_half = [], dt.host

    def recording_host(batch, index=None):
        out = host_half(batch, index)
        planned.append(out["plans"].clone())
        return out

    dt.host = recording_host
    raw = list(train)
    got = list(DevicePrefetcher(train, DEV))
    torch.cuda.synchronize()
    assert len(got) == len(planned) == 4
    mean, std = MEAN.to(DEV), STD.to(DEV)
    for src, plans, b in zip(raw, planned, got):
        assert set(b) == set(src) and "plans" not in b                       # the usual keys reach the model
        assert b["video"].is_cuda and b["video"].dtype == torch.float32 and b["video"].shape == (2, 3, 3, 64, 96)
        assert torch.equal(b["video"], ops.clip_crop_resize(src["video"].to(DEV), plans.to(DEV), (64, 96), mean, std))
        host = b["_host_annotations"]
        for k in ("boxes", "classes", "active"):
            assert not host[k].is_cuda and torch.equal(b[k].cpu(), host[k])
        act = host["active"].bool()
        bx = host["boxes"][act]
        assert len(bx) and float(bx.min()) >= 0 and float(bx[:, [0, 2]].max()) <= 96 and float(bx[:, [1, 3]].max()) <= 64
        assert not host["boxes"][~act].any()
        assert (plans[:, 2] >= 45).all() and (plans[:, 2] <= 90).all() and (plans[:, 4] == 0).all()
    assert all(not torch.equal(p, q) for p, q in zip(planned, planned[1:]))   # consecutive batches, other rectangles
    assert len({tuple(p.flatten().tolist()) for p in planned}) == 4
    # the validation loader: the centre crop, exactly the raw pixels
    (vb,), (vraw,) = list(DevicePrefetcher(val["val"], DEV)), list(val["val"])
    want = ((vraw["video"][..., 13:77, 32:128].float() / 255) - MEAN.view(3, 1, 1)) / STD.view(3, 1, 1)
    assert torch.equal(vb["video"].cpu(), want)

    # a few captured steps: ONE capture, finite losses
    model, opt = _build()
    step = GraphedStep(model, opt, warmup=2)
    losses = [float(step(b)[1].detach()) for b in DevicePrefetcher(train, DEV)]
    assert step.replays == 4 and len(step._graphs) == 1
    assert all(l == l and abs(l) < 1e6 for l in losses), losses
    assert len(planned) == 8 and not torch.equal(planned[4], planned[0])      # the second epoch crops anew


def test_trainer_short_run_with_augmenting_loaders(tmp_path):
    from future_od.models.st_detr import SpatioTemporalDETRArgs
    from future_od.trainer import Trainer
    from runs._helper import get_lr_func, setup_optimizer
    from runs._model import build_model
    torch.manual_seed(0)
    args = SimpleNamespace(device=DEV, distributed=False, compute_dtype="bf16", backbone="resnet18")
    detr = SpatioTemporalDETRArgs(num_classes=8, num_queries=32, lr_backbone=1e-4, enc_layers=1, dec_layers=2,
                                  pretrained_backbone=False)
    model = build_model(args, detr)
    sched, opt = setup_optimizer(detr, model, get_lr_func(4))
    train, val = _aug_loaders(steps=3)
    tr = Trainer(model, opt, sched, train, val, str(tmp_path), str(tmp_path), "t", DEV, print_interval=3,
                 visualization_epochs=[], visualization_iterations=[], category_dict={}, checkpoint_epochs=True,
                 is_master=True, max_norm=detr.max_norm)
    tr.train(2)
    assert tr._graphed not in (None, False) and tr._graphed.replays == 6 and len(tr._graphed._graphs) == 1
    assert tr._graphed_eval not in (None, False) and tr._graphed_eval.replays == 2 and len(tr._graphed_eval._graphs) == 1
    assert opt._step_no == 6 and tr._training_iterations == 6
    hist = tr._stats["train labels loss"].history
    assert len(hist) == 2 and all(h == h for h in hist)
    assert train.device_transform._index == 6 and val["val"].device_transform._index == 2
