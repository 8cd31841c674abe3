"""Attention maps on the device: fod_attn_maps against the float64 reference of tests/attention_map_cases.py at its edges,
fod_render_attention byte for byte against the numpy restatement, and the public surface -- predict(attention=True),
GraphedPredict(attention=True), stored_attention -- on the small test model of test_predict_gpu.py."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import attention_map_cases as AC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -7.0


def _dev(t):
    """The tensor on the device with the strides it has on the host (a column slot stays a column slot)."""
    if t is None:
        return None
    return torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=DEV).copy_(t)


def _launch(jobs, scale, idx, B, Q, S):
    from future_od.native import ops
    out = torch.full((B, Q, len(jobs), S), SENTINEL, dtype=torch.float32, device=DEV)
    got = ops.attn_maps([tuple(_dev(t) for t in job) for job in jobs], scale, None if idx is None else idx.to(DEV), out=out)
    assert got is out
    return out


def _check_maps(got, ref, valid, lim, what):
    """Distance to the reference, row sums and padded rows of one launch's output (a host copy)."""
    assert bool(torch.isfinite(got).all()) and not bool((got == SENTINEL).any()), what     # every element was written
    d = AC.distance(got, ref, valid)
    sums = float((got.double().sum(-1) - 1.0).abs()[valid].max()) if bool(valid.any()) else 0.0
    print(f"{what}: distance {d:.3e}, row sums off by {sums:.3e}, limit {lim:.3e}")
    assert d <= lim, (what, d, lim)
    assert sums <= lim, (what, sums, lim)
    assert not bool(got[~valid].any()), what                                               # padded rows: exactly zero


@pytest.mark.parametrize("name", list(AC.BY_NAME))
def test_attn_maps_against_float64(name):
    case = AC.BY_NAME[name]
    jobs, scale, idx = AC.build(case)
    ref, A = AC.reference(jobs, scale, case.H, idx)
    assert tuple(ref.shape) == (case.B, case.Q, case.njobs, case.S)
    valid = AC.valid_rows(idx, case.B, case.Q, case.Tq)
    first = _launch(jobs, scale, idx, case.B, case.Q, case.S)
    second = _launch(jobs, scale, idx, case.B, case.Q, case.S)
    assert torch.equal(first, second)                                                      # two launches: equal bits
    _check_maps(first.cpu(), ref, valid, AC.limit(AC.D32[name], A), name)


def test_attn_maps_wrapper_refuses_bad_operands():
    from future_od.native import lib as L
    from future_od.native import ops
    q, k = torch.zeros(2, 5, 64, dtype=torch.bfloat16, device=DEV), torch.zeros(2, 7, 64, dtype=torch.bfloat16, device=DEV)
    idx = torch.zeros(2, 3, dtype=torch.int32, device=DEV)
    for bad in (lambda: ops.attn_maps([], 0.1), lambda: ops.attn_maps([(q, None, k, None)] * 33, 0.1),
                lambda: ops.attn_maps([(q, q, k, None)], 0.1), lambda: ops.attn_maps([(q, None, k, None), (q, q, k, k)], 0.1),
                lambda: ops.attn_maps([(q, None, k, None), (q, None, k[:, :6], None)], 0.1),
                lambda: ops.attn_maps([(q, None, k.float(), None)], 0.1),
                lambda: ops.attn_maps([(q.cpu(), None, k.cpu(), None)], 0.1),
                lambda: ops.attn_maps([(q, None, k, None)], 0.1, idx.long()), lambda: ops.attn_maps([(q, None, k, None)], 0.1, idx[:1]),
                lambda: ops.attn_maps([(q, None, k, None)], 0.1, idx, out=torch.zeros(2, 3, 1, 8, device=DEV))):
        with pytest.raises(L.FodError):
            bad()


# ---- the overlay --------------------------------------------------------------------------------------------------------
OVERLAY = AC.overlay_cases()


@pytest.mark.parametrize("case", OVERLAY, ids=[c["name"] for c in OVERLAY])
def test_render_attention_gives_the_restated_bytes(case):
    from future_od.utils import visualization as V
    video, att = torch.from_numpy(case["video"]).to(DEV), torch.from_numpy(case["attention"]).to(DEV)
    slot = case["slot"] if isinstance(case["slot"], int) else torch.from_numpy(case["slot"]).to(DEV)
    got = V.render_attention(video, att, torch.tensor(case["frames"], dtype=torch.int32), slot, case["gain"], case["max_alpha"])
    want = AC.overlay_expected(case)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy(), want), int((got.cpu().numpy() != want).sum())
    if case["gain"] == 0.0 or case["max_alpha"] == 0.0:                                    # the plain frame: render, no boxes
        B, J = want.shape[:2]
        for j, f in enumerate(case["frames"]):
            plain = V.render(video, torch.zeros(B, 0, 4, device=DEV), torch.zeros(B, 0, dtype=torch.int32, device=DEV),
                             frame_idx=torch.full((B,), f, dtype=torch.int32))
            assert torch.equal(got[:, j], plain)


def test_render_attention_writes_into_a_sentinel_filled_destination_and_takes_strided_maps():
    from future_od.native import ops
    from future_od.utils import visualization as V
    case = next(c for c in OVERLAY if c["name"].startswith("small") and "u8" not in c["name"])
    video, att = torch.from_numpy(case["video"]).to(DEV), torch.from_numpy(case["attention"]).to(DEV)
    B, K, J = att.shape[:3]
    maps = att[:, case["slot"]]                                                            # a view: strides over b and j
    assert not maps.is_contiguous()
    cs = (1.0 / maps.amax(dim=(2, 3)).clamp_min(1e-30)).contiguous()
    frames = torch.tensor(case["frames"], dtype=torch.int32, device=DEV)[None].expand(B, J).contiguous()
    _, mean, std = V._device_constants(video.device)
    out = torch.full((B, J) + tuple(video.shape[-2:]) + (3,), 99, dtype=torch.uint8, device=DEV)
    got = ops.render_attention(video, maps, frames, cs, mean=mean, std=std, lut=V.ATTENTION_LUT.to(DEV), out=out)
    assert got is out and np.array_equal(out.cpu().numpy(), AC.overlay_expected(case))


# ---- the model ----------------------------------------------------------------------------------------------------------
OLD_KEYS = ("scores", "labels", "boxes", "query", "count")


def _data(seed=11):
    from future_od.datasets.synthetic import make_batch
    from test_predict_gpu import _strip
    return _strip(make_batch(2, 3, 96, 128, seed=seed, max_boxes=9, device=DEV))


def _variant(**kw):
    """The small model with other architecture options (random weights)."""
    from future_od.models.st_detr import SpatioTemporalDETRArgs
    from runs._model import build_model
    torch.manual_seed(5)
    args = SimpleNamespace(device=DEV, distributed=False, compute_dtype="bf16", backbone="resnet18", **kw)
    detr = SpatioTemporalDETRArgs(num_classes=8, num_queries=128, lr_backbone=1e-4, enc_layers=1, dec_layers=2,
                                  pretrained_backbone=False)
    return build_model(args, detr).eval()


def _tapped_operands(model, data):
    """The operands of the last decoder layer's cross-attention blocks in one more pass of the core, on the host."""
    from future_od.models.transformer import AttentionTap
    core = model._model
    tap = core.attention_tap = AttentionTap()
    try:
        with torch.no_grad():
            core(data["video"], **model._core_kwargs(data))
    finally:
        core.attention_tap = None
    jobs = []
    for image in sorted(tap.blocks):
        qc, qs, side, layer, im = tap.blocks[image]
        assert layer == len(core.detector.decoder.layers) - 1 and im == image
        kc, ks, _v = side.slots(layer, image)
        jobs.append(tuple(t.detach().cpu() for t in (qc, qs, kc, ks)))
    return jobs, tap


def _reference_for(model, data, query):
    jobs, tap = _tapped_operands(model, data)
    D = jobs[0][0].shape[-1]
    H = model._model.detector.decoder.layers[-1].self_attend.Nhead
    scale = 1.0 / math.sqrt(2 * D // H)
    idx = query.cpu()
    ref, A = AC.reference(jobs, scale, H, idx)
    f32, _ = AC.reference([tuple(t.float() for t in job) for job in jobs], scale, H, idx, torch.float32)
    valid = AC.valid_rows(idx, idx.shape[0], idx.shape[1], jobs[0][0].shape[1])
    return ref, AC.limit(AC.distance(f32, ref, valid), A), valid, tap


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_predict_with_attention_adds_two_keys_and_changes_nothing_else(dtype):
    from future_od.native import lib as L
    from test_graph_gpu import _build
    model, _ = _build(dtype)
    data = _data()
    # a threshold that the 31st detection of one sample just meets: rows that hold a detection and padding rows
    thr = float(model.predict(data, top_k=40)["scores"][:, 30].max())
    L.PROFILER.start()
    plain = model.predict(data, top_k=40, score_threshold=thr)
    launches = [r[0] for r in L.PROFILER.records]
    L.PROFILER.start()
    det = model.predict(data, top_k=40, score_threshold=thr, attention=True)
    tapped = [r[0] for r in L.PROFILER.records]
    L.PROFILER.start()
    again = model.predict(data, top_k=40, score_threshold=thr)
    after = [r[0] for r in L.PROFILER.records]
    L.PROFILER.stop()
    assert set(plain) == set(again) == set(OLD_KEYS) and set(det) == set(OLD_KEYS) | {"attention", "attention_frames"}
    assert all(torch.equal(det[k], plain[k]) and torch.equal(again[k], plain[k]) for k in OLD_KEYS)
    assert "fod_attn_maps" not in launches and tapped == launches + ["fod_attn_maps"] and after == launches
    core = model._model
    assert core.attention_tap is None and all(b.attention_tap is None for layer in core.detector.decoder.layers
                                              for b in layer.image_attend)
    att, frames = det["attention"], det["attention_frames"]
    assert att.is_cuda and att.dtype == torch.float32 and tuple(att.shape) == (2, 40, 2, 3, 4)
    assert frames.is_cuda and frames.dtype == torch.int32 and frames.tolist() == [1, 0]
    assert 0 < int(det["count"].sum()) < 80                                               # real rows and padding rows
    ref, lim, valid, _ = _reference_for(model, data, det["query"])
    assert torch.equal(valid, (torch.arange(40)[None] < det["count"].cpu()[:, None]))
    _check_maps(att.cpu().flatten(3), ref, valid, lim, f"predict {dtype}")


def test_graphed_predict_with_attention_replays_the_eager_bits():
    from future_od.graph import GraphedPredict
    from test_graph_gpu import _build
    model, _ = _build("bf16")
    data, data2 = _data(11), _data(12)
    gp = GraphedPredict(model, top_k=50, score_threshold=0.05, attention=True)
    for d in (data, data2, data):
        want = model.predict(d, top_k=50, score_threshold=0.05, attention=True)
        got = gp(d)
        assert set(got) == set(want) == set(OLD_KEYS) | {"attention", "attention_frames"}
        assert all(torch.equal(got[k], want[k]) for k in want)
        assert float(got["attention"].sum()) > 0
    assert len(gp._graphs) == 1 and gp.replays == 3
    assert set(GraphedPredict(model, top_k=50)(data)) == set(OLD_KEYS)                     # the option is off by default


def test_stored_attention_on_the_device_is_the_launch_with_all_queries():
    from future_od.native import ops
    from test_graph_gpu import _build
    model, _ = _build("bf16")
    data = _data()
    block = model._model.detector.decoder.layers[-1].image_attend[1]
    block.store_attention = True
    try:
        jobs, tap = _tapped_operands(model, data)
    finally:
        block.store_attention = False
    stored = block.stored_attention
    assert stored.is_cuda and stored.dtype == torch.float32 and tuple(stored.shape) == (2, 128, 12)
    D, H = 256, block.Nhead
    direct = ops.attn_maps([tuple(t.to(DEV) for t in jobs[1])], 1.0 / math.sqrt(2 * D // H))
    assert torch.equal(direct[:, :, 0], stored)
    ref, A = AC.reference(jobs[1:], 1.0 / math.sqrt(2 * D // H), H)
    f32, _ = AC.reference([tuple(t.float() for t in jobs[1])], 1.0 / math.sqrt(2 * D // H), H, None, torch.float32)
    valid = torch.ones(2, 128, dtype=torch.bool)
    _check_maps(stored.cpu()[:, :, None], ref, valid, AC.limit(AC.distance(f32, ref, valid), A), "stored_attention")


def test_all_at_once_memory_comes_back_split_into_its_frames():
    model = _variant(num_images=1, image_memory_mode="attend all at once", no_temporal=False)
    data = _data()
    det = model.predict(data, top_k=30, attention=True)
    att = det["attention"]
    assert tuple(att.shape) == (2, 30, 2, 3, 4) and det["attention_frames"].tolist() == [0, 1]
    ref, lim, valid, tap = _reference_for(model, data, det["query"])
    assert tap.split == 2 and tuple(ref.shape) == (2, 30, 1, 24) and bool(valid.all())
    got = att.cpu().flatten(2)[:, :, None]                                                 # [B, K, 1, keep * N]
    _check_maps(got, ref, valid, lim, "all at once")                                       # sums to 1 over BOTH images
    per_image = att.sum(dim=(3, 4))
    assert bool((per_image < 1.0).all()) and bool((per_image > 0.0).all())


def test_f2f_model_has_no_maps():
    model = _variant(joint_mode="f2f", joint_f2f_frames=2)
    data = _data()
    assert set(model.predict(data, top_k=10)) == set(OLD_KEYS)
    with pytest.raises(ValueError, match="JointEncoderF2F"):
        model.predict(data, top_k=10, attention=True)
    assert model._model.attention_tap is None
    assert set(model.predict(data, top_k=10)) == set(OLD_KEYS)
