"""Label-free inference on the device: fod_detect_select against the project's own post-processing (bit for bit),
SpatioTemporalDETR.predict against forward, GraphedPredict against eager predict, and the raw-frame path whose boxes
come back in camera pixels."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H, W = 448, 800
SENTINELS = (7.0, 77, 7.0, 77, 77)


def _logits(kind, B, M, C, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "randn":
        return 3 * torch.randn(B, M, C, generator=g)
    if kind == "four":                                         # many exact ties: the index order decides
        return torch.tensor([-2.0, -0.25, 0.5, 3.0])[torch.randint(0, 4, (B, M, C), generator=g)]
    if kind == "equal":
        return torch.full((B, M, C), 0.75)
    if kind == "special":                                      # NaN is never selected, +inf scores 1, -inf scores 0
        x = 3 * torch.randn(B, M, C, generator=g)
        r = torch.rand(B, M, C, generator=g)
        x[r < 0.15] = float("nan")
        x[(r >= 0.15) & (r < 0.25)] = float("inf")
        x[(r >= 0.25) & (r < 0.4)] = float("-inf")
        x[:, 0] = float("nan")                                 # a query with nothing but NaN
        return x
    raise ValueError(kind)


def _boxes(B, M, seed):
    g = torch.Generator().manual_seed(seed + 1)
    return torch.cat([0.1 + 0.8 * torch.rand(B, M, 2, generator=g), 0.02 + 0.4 * torch.rand(B, M, 2, generator=g)], dim=2)


def _expected(logits, boxes, K, thr, per_query):
    """The selection, restated with torch on the host copies of ops.post_proc's outputs."""
    from future_od.native import ops
    s, bp = (t.cpu() for t in ops.post_proc(logits.to(DEV), boxes.to(DEV), H, W))
    B, M, C = logits.shape
    scores, labels = torch.zeros(B, K), torch.full((B, K), -1, dtype=torch.int32)
    query, out_boxes = torch.full((B, K), -1, dtype=torch.int32), torch.zeros(B, K, 4)
    count = torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        if per_query:
            cand = s[b, :, C]
            first = ((s[b, :, :C] == cand[:, None]).cumsum(1) == 0).sum(1)          # lowest class that attains the maximum
            q, c = torch.arange(M), first
        else:
            cand = s[b, :, :C].reshape(-1)
            q, c = torch.arange(M * C) // C, torch.arange(M * C) % C
        eligible = cand >= torch.tensor(thr, dtype=torch.float32)                    # a NaN compares false
        if per_query:
            eligible &= cand >= 0                                                    # (the "maximum" of an all-NaN query is -inf)
        _, order = torch.sort(torch.where(eligible, cand, torch.tensor(-1.0)), stable=True, descending=True)
        n = min(K, int(eligible.sum()))
        take = order[:n]
        assert bool(eligible[take].all())
        count[b] = n
        scores[b, :n], labels[b, :n], query[b, :n] = cand[take], c[take].int(), q[take].int()
        out_boxes[b, :n] = bp[b, q[take]]
    return scores, labels, out_boxes, query, count


def _select(logits, boxes, K, thr, per_query, box_map=None):
    from future_od.native import ops
    B = logits.shape[0]
    out = (torch.full((B, K), SENTINELS[0], device=DEV), torch.full((B, K), SENTINELS[1], dtype=torch.int32, device=DEV),
           torch.full((B, K, 4), SENTINELS[2], device=DEV), torch.full((B, K), SENTINELS[3], dtype=torch.int32, device=DEV),
           torch.full((B,), SENTINELS[4], dtype=torch.int32, device=DEV))
    got = ops.detect_select(logits.to(DEV), boxes.to(DEV), H, W, K, thr, per_query,
                            None if box_map is None else box_map.to(DEV), out=out)
    assert all(g is o for g, o in zip(got, out))
    return tuple(t.cpu() for t in got)


def _check(logits, boxes, K, thr, per_query):
    want = _expected(logits, boxes, K, thr, per_query)
    got = _select(logits, boxes, K, thr, per_query)
    for name, g, w in zip(("scores", "labels", "boxes", "query", "count"), got, want):
        assert g.dtype == w.dtype and torch.equal(g, w), (name, g, w)
    return got


SHAPES = [(1, 1, 1, 1), (3, 5, 3, 4), (3, 5, 3, 15), (3, 5, 3, 20), (2, 128, 9, 100), (2, 128, 9, 1024), (1, 1024, 8, 1024)]


@pytest.mark.parametrize("per_query", [False, True])
@pytest.mark.parametrize("kind", ["randn", "four", "equal"])
@pytest.mark.parametrize("shape", SHAPES)
def test_detect_select_matches_post_proc_bit_for_bit(shape, kind, per_query):
    B, M, C, K = shape
    logits, boxes = _logits(kind, B, M, C, seed=M * 31 + C), _boxes(B, M, seed=M)
    scores, labels, _, query, count = _check(logits, boxes, K, 0.0, per_query)
    n = M if per_query else M * C
    assert count.tolist() == [min(K, n)] * B
    if kind == "equal":                                        # nothing but ties: the first K flat indices
        k = min(K, n)
        flat = query[:, :k] if per_query else query[:, :k] * C + labels[:, :k]
        assert torch.equal(flat, torch.arange(k, dtype=torch.int32).repeat(B, 1))
        assert not per_query or int(labels[:, :k].max()) == 0


@pytest.mark.parametrize("per_query", [False, True])
@pytest.mark.parametrize("shape", [(3, 5, 3, 15), (2, 128, 9, 100)])
def test_detect_select_thresholds(shape, per_query):
    from future_od.native import ops
    B, M, C, K = shape
    logits, boxes = _logits("randn", B, M, C, seed=5), _boxes(B, M, seed=5)
    logits[0, 1] = logits[0, 0]                                # the threshold below is met by more than one candidate
    s, _ = ops.post_proc(logits.to(DEV), boxes.to(DEV), H, W)
    col = s[0, :, C] if per_query else s[0, :, :C].reshape(-1)
    existing = float(col.cpu().sort().values[col.numel() // 2])                     # a score that occurs: inclusive
    _, _, _, _, count = _check(logits, boxes, K, existing, per_query)
    assert int(count[0]) == min(K, int((col.cpu() >= existing).sum())) and 0 < int(count[0])
    _, _, _, _, count = _check(logits, boxes, K, 1.1, per_query)
    assert count.tolist() == [0] * B
    _, _, _, _, count = _check(logits, boxes, K, -0.5, per_query)
    assert count.tolist() == [min(K, M if per_query else M * C)] * B


@pytest.mark.parametrize("per_query", [False, True])
@pytest.mark.parametrize("thr", [0.0, -1.0, 0.5, 1.0])
@pytest.mark.parametrize("shape", [(3, 5, 3, 15), (2, 128, 9, 1024)])
def test_detect_select_nan_and_infinite_logits(shape, thr, per_query):
    B, M, C, K = shape
    logits, boxes = _logits("special", B, M, C, seed=9), _boxes(B, M, seed=9)
    scores, labels, _, query, count = _check(logits, boxes, K, thr, per_query)
    assert not torch.isnan(scores).any() and int(count.sum()) > 0
    for b in range(B):
        n = int(count[b])
        if n == 0:
            continue
        picked = logits[b, query[b, :n].long(), labels[b, :n].long()]
        assert not torch.isnan(picked).any() and int(query[b, :n].min()) > 0        # query 0 is all NaN
        assert bool((scores[b, :n][picked == float("inf")] == 1).all())
        if thr > 0:
            assert not (picked == float("-inf")).any()
        elif not per_query and n < K:                                                # everything eligible fits: -inf is in, score 0
            assert int((picked == float("-inf")).sum()) == int((logits[b] == float("-inf")).sum())


def test_detect_select_box_map():
    B, M, C, K = 3, 40, 5, 64
    logits, boxes = _logits("randn", B, M, C, seed=2), _boxes(B, M, seed=2)
    plain = _select(logits, boxes, K, 0.3, False)
    ident = _select(logits, boxes, K, 0.3, False, torch.tensor([[1.0, 1.0, 0.0, 0.0]]).repeat(B, 1))
    for g, w in zip(ident, plain):
        assert torch.equal(g, w)                                                     # the bits of NULL
    # per-sample maps, two with sx < 0 (a flip); |coordinates| stay below 2048
    maps = torch.tensor([[-1.25, 0.7, 1900.0, 100.0], [2.3, 1.9, 33.0, -7.5], [-0.4, 2.1, 320.5, 12.25]])
    got = _select(logits, boxes, K, 0.3, False, maps)
    for i in (0, 1, 3, 4):
        assert torch.equal(got[i], plain[i])
    n = int(plain[4].min())
    assert n > 8
    b64, m64 = plain[2].double(), maps.double()[:, None, :]
    xa, xb = b64[..., 0] * m64[..., 0] + m64[..., 2], b64[..., 2] * m64[..., 0] + m64[..., 2]
    ya, yb = b64[..., 1] * m64[..., 1] + m64[..., 3], b64[..., 3] * m64[..., 1] + m64[..., 3]
    want = torch.stack([torch.minimum(xa, xb), torch.minimum(ya, yb), torch.maximum(xa, xb), torch.maximum(ya, yb)], dim=2)
    assert float(want.abs().max()) < 2048
    for b in range(B):
        k = int(plain[4][b])
        err = float((got[2][b, :k].double() - want[b, :k]).abs().max())
        assert err <= 2e-3, (b, err)                           # three f32 roundings of at most 2.4e-4 each
        assert bool((got[2][b, :k, 0] <= got[2][b, :k, 2]).all() and (got[2][b, :k, 1] <= got[2][b, :k, 3]).all())
        assert not got[2][b, k:].any()                         # padding rows stay zero, whatever the map's offset


def test_detect_select_refuses_bad_operands():
    from future_od.native import lib as L
    from future_od.native import ops
    lg, bx = torch.zeros(2, 4, 3, device=DEV), torch.zeros(2, 4, 4, device=DEV)
    for bad in (lambda: ops.detect_select(lg, bx, H, W, 0), lambda: ops.detect_select(lg, bx, H, W, 1025),
                lambda: ops.detect_select(lg.double(), bx, H, W, 4), lambda: ops.detect_select(lg, bx[:, :3], H, W, 4),
                lambda: ops.detect_select(lg, bx, H, W, 4, box_map=torch.zeros(1, 4, device=DEV)),
                lambda: ops.detect_select(lg, bx, H, W, 4, box_map=torch.zeros(2, 4)),
                lambda: ops.detect_select(torch.zeros(1, 8193, 1, device=DEV), torch.zeros(1, 8193, 4, device=DEV), H, W, 4)):
        with pytest.raises(L.FodError):
            bad()


# ---- the model ----------------------------------------------------------------------------------------------------
ANNOTATION_KEYS = ("boxes", "classes", "active", "ignore_boxes", "annotated_frame_idx")


def _strip(data):
    return {k: v for k, v in data.items() if k not in ANNOTATION_KEYS + ("_host_annotations",)}


def _same(a, b):
    return set(a) == set(b) == {"scores", "labels", "boxes", "query", "count"} and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_predict_is_the_detector_of_forward(dtype):
    from future_od.datasets.synthetic import make_batch
    from test_graph_gpu import _build
    model, _ = _build(dtype)
    data = make_batch(2, 3, 96, 128, seed=11, max_boxes=9, device=DEV)
    with torch.no_grad():
        post = model(data=data, distributed=False)[0]
    cs, bp = post["class_scores"][:, 0, 0], post["boxes"][:, 0, 0]                   # [B,M,C+1], [B,M,4]
    for per_query, K in ((False, 100), (True, 40)):
        det = model.predict(data, top_k=K, per_query=per_query)
        assert det["scores"].shape == (2, K) and det["labels"].dtype == det["query"].dtype == det["count"].dtype == torch.int32
        assert det["count"].tolist() == [K, K] and all(v.is_cuda for v in det.values())
        q, c = det["query"].long(), det["labels"].long()
        bi = torch.arange(2, device=DEV)[:, None]
        assert torch.equal(cs[bi, q, c], det["scores"]) and torch.equal(bp[bi, q], det["boxes"])
        if per_query:
            assert torch.equal(cs[bi, q, 8], det["scores"])
        assert bool((det["scores"][:, :-1] >= det["scores"][:, 1:]).all())
        stripped = _strip(data)
        assert not set(stripped) & set(ANNOTATION_KEYS)
        assert _same(model.predict(stripped, top_k=K, per_query=per_query), det)
    with pytest.raises(KeyError):
        model(data=_strip(data), distributed=False)
    model.train()
    with pytest.raises(RuntimeError, match="evaluation only"):
        model.predict(data)


def test_graphed_predict_replays_eager_predict():
    from future_od.datasets.synthetic import make_batch
    from future_od.graph import GraphedPredict
    from test_graph_gpu import _build, _eager_step
    model, opt = _build("bf16")
    data = make_batch(2, 3, 96, 128, seed=11, max_boxes=9, device=DEV)
    data2 = make_batch(2, 3, 96, 128, seed=12, max_boxes=20, device=DEV)
    free = _strip(data)
    gp = GraphedPredict(model, top_k=50, score_threshold=0.05)
    want = model.predict(free, top_k=50, score_threshold=0.05)
    assert _same(gp(free), want)
    assert _same(gp(_strip(data2)), model.predict(data2, top_k=50, score_threshold=0.05))
    assert len(gp._graphs) == 1 and gp.replays == 2
    (g,) = gp._graphs.values()
    assert set(g["static"]) == set(model.predict_inputs(free)) and g["record"].of("prepared operands")
    for _ in range(2):                                          # the parameters move: the graph reads the new ones
        _eager_step(model, opt, data)
    moved = model.predict(free, top_k=50, score_threshold=0.05)
    assert not _same(moved, want)
    assert _same(gp(free), moved)
    assert _same(gp(data), moved) and len(gp._graphs) == 1      # label keys are ignored: same graph, nothing staged for them
    mapped = dict(free, box_map=torch.tensor([[-1.0, 1.0, 128.0, 0.0], [2.0, 2.0, 5.0, 7.0]], device=DEV))
    got = gp(mapped)
    assert len(gp._graphs) == 2 and _same(got, model.predict(mapped, top_k=50, score_threshold=0.05))
    assert not torch.equal(got["boxes"], moved["boxes"]) and torch.equal(got["scores"], moved["scores"])
    model.train()
    with pytest.raises(RuntimeError, match="evaluation only"):
        gp(free)


class _Loader(list):
    batch_size = 2


def _raw_free(seed):
    from future_od.datasets.synthetic import make_batch
    return _strip(make_batch(2, 3, 120, 160, seed=seed, raw_frames=True))


def test_raw_label_free_frames_give_boxes_in_camera_pixels():
    import future_od.datasets.transforms as T
    from future_od.utils.augment import DeviceJointTransform
    from future_od.utils.prefetch import DevicePrefetcher
    from test_graph_gpu import _build
    model, _ = _build("bf16")
    # a centre crop: the camera's pixels are the crop's plus (left, top)
    loader = _Loader([_raw_free(31)])
    loader.device_transform = DeviceJointTransform(T.JointCompose([T.JointCenterCrop((96, 128))]))
    (batch,) = list(DevicePrefetcher(loader, DEV))
    assert batch["video"].shape == (2, 3, 3, 96, 128) and batch["video"].dtype == torch.float32
    assert not set(batch) & set(ANNOTATION_KEYS + ("_host_annotations", "plans", "_plan_size"))
    assert torch.equal(batch["box_map"].cpu(), torch.tensor([[1.0, 1.0, 16.0, 12.0]]).repeat(2, 1))
    det = model.predict(batch, top_k=30)
    base = model.predict({k: v for k, v in batch.items() if k != "box_map"}, top_k=30)
    assert torch.equal(det["scores"], base["scores"]) and torch.equal(det["query"], base["query"])
    shift = torch.tensor([16.0, 12.0, 16.0, 12.0], device=DEV)
    assert float((det["boxes"] - (base["boxes"] + shift)).abs().max()) <= 2e-3
    # crop, resize and flip: against the float64 map
    loader = _Loader([_raw_free(32)])
    t = T.JointCompose([T.JointCenterCrop((96, 128)), T.JointResize((64, 96)), T.JointHorizontalFlip(1.0)])
    loader.device_transform = DeviceJointTransform(t)
    (batch,) = list(DevicePrefetcher(loader, DEV))
    assert batch["video"].shape == (2, 3, 3, 64, 96)
    sx, sy, ox, oy = t.plan(120, 160).box_map()
    assert (sx, sy, ox, oy) == (-128 / 96, 1.5, 144.0, 12.0)
    det = model.predict(batch, top_k=30)
    base = model.predict({k: v for k, v in batch.items() if k != "box_map"}, top_k=30)["boxes"].double()
    sx32 = float(torch.tensor(sx, dtype=torch.float32))                              # the map travels as f32
    want = torch.stack([base[..., 2] * sx32 + ox, base[..., 1] * sy + oy, base[..., 0] * sx32 + ox, base[..., 3] * sy + oy], dim=2)
    assert float((det["boxes"].double() - want).abs().max()) <= 2e-3
    assert bool((det["boxes"][..., 0] <= det["boxes"][..., 2]).all())
