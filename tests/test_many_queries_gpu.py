"""More than 256 queries on the device: fod_lap_solve_batch_dev's second launch form (state for 1024 rows and columns,
every workgroup staging its own n * M costs in LDS when they fit) against the host solver and scipy, the criterion and
the whole model -- eager, captured, inference -- at Conditional DETR's default of 300 queries, and the launch shapes that
only a 300-query decoder produces (Tq = S = 300 attention through the key split, 600-row fused launches)."""
import numpy as np
import pytest
import torch

from future_od import switches
from future_od.native import abi
from test_many_queries_cpu import assert_equals_scipy, tie_costs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STAGE = abi.CONSTANTS["FOD_LAP_STAGE_FLOATS"]
LAST_STAGED = STAGE // 300                    # largest n whose n x 300 problem is solved from LDS

if torch.cuda.is_available():
    from future_od.native import ops


# ---- the solver ---------------------------------------------------------------------------------------------------
def _solve_and_compare(M, sizes, ld, Lv):
    """The device's matches equal the host solver's plus the offsets, bit for bit, and scipy's (i, j); status stays 0."""
    B = len(sizes)
    assert B == 2
    cost = tie_costs(M, ld, Lv, seed=M * 7919 + sum(sizes) * 31 + ld)
    off = [0, sizes[0], sizes[0] + sizes[1]]
    off_dev = torch.tensor(off, dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = ops.lap_solve_batch_dev(cost.to(DEV), off_dev, status).cpu()
    assert int(status.item()) == 0
    host = ops.lap_solve_batch_host(cost.view(Lv * B, M, ld).contiguous(), sizes * Lv, threads=4).view(Lv, B, M)
    for lv in range(Lv):
        for b in range(B):
            want = torch.where(host[lv, b] >= 0, host[lv, b] + off[b], host[lv, b])
            assert torch.equal(got[lv, b], want), (lv, b, sizes[b])
            if sizes[b]:
                mine = got[lv, b]
                assert_equals_scipy(torch.where(mine >= 0, mine - off[b], mine), cost[lv, b], sizes[b])


LARGE_FORM = [(257, [1, 256], 256, 3), (300, [37, 0], 256, 3), (300, [256, 5], 256, 3), (300, [300, 299], 300, 3),
              (512, [512, 3], 512, 3), (1024, [17, 256], 256, 3), (1024, [1024, 1], 1024, 1),
              (300, [LAST_STAGED, LAST_STAGED + 1], 256, 3)]      # one launch, one problem on either side of the limit


@pytest.mark.parametrize("case", LARGE_FORM, ids=lambda c: f"M{c[0]}-n{c[1][0]}+{c[1][1]}-ld{c[2]}")
def test_device_solver_beyond_256_is_bit_identical_to_the_host_solver_and_scipy(case):
    M, sizes, ld, Lv = case
    assert M > 256 or ld > 256                                     # the workgroup-staged form
    assert LAST_STAGED * 300 <= STAGE < (LAST_STAGED + 1) * 300 and LAST_STAGED + 1 <= 256
    _solve_and_compare(M, sizes, ld, Lv)


def test_device_solver_at_256_with_costs_in_global_memory():
    """The host-staged form's cost-in-global branch (256 x 256 costs do not fit beside the state): code that the
    128-query tests never reach."""
    _solve_and_compare(256, [256, 200], 256, 3)


def test_device_solver_status_words_at_300_queries():
    M, ld = 300, 256
    cost = tie_costs(M, ld, 1, seed=5)                             # [1, 2, M, ld]
    clean = cost.clone()
    cost[0, 1, 17, 3] = float("nan")
    off = torch.tensor([0, 9, 21], dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = ops.lap_solve_batch_dev(cost.to(DEV), off, status).cpu()
    assert int(status.item()) == 1 and bool((got[0, 1] == -1).all())
    host = ops.lap_solve_batch_host(clean[0, :1].contiguous(), [9], threads=1)[0]
    assert torch.equal(got[0, 0], host)                            # the other problem of the launch is solved (offset 0)
    # a NaN beyond the valid columns is not part of any problem
    cost = clean.clone()
    cost[0, 1, 17, 12] = float("nan")
    status.zero_()
    got = ops.lap_solve_batch_dev(cost.to(DEV), off, status).cpu()
    assert int(status.item()) == 0 and int((got[0, 1] >= 0).sum()) == 12
    # offsets that claim more targets than the cost matrix has columns
    off = torch.tensor([0, 4, 4 + ld + 1], dtype=torch.int32, device=DEV)
    status.zero_()
    got = ops.lap_solve_batch_dev(clean.to(DEV), off, status).cpu()
    assert int(status.item()) == 2 and bool((got[0, 1] == -1).all()) and int((got[0, 0] >= 0).sum()) == 4


# ---- the criterion ------------------------------------------------------------------------------------------------
def test_device_target_path_equals_host_matcher_at_300_queries():
    """test_device_target_path_equals_host_matcher with logits [3, 3, 300, 8]: packed, matched and normalised on the device
    against the host path, equal loss tables and gradients."""
    from future_od.models.set_criterion import SetCriterion, build_matcher
    from future_od.models.st_detr import SpatioTemporalDETRArgs, to_detr_targets
    from test_heads_gpu import _criterion_inputs
    crit = SetCriterion(8, build_matcher(SpatioTemporalDETRArgs(num_classes=8)), {}, 0.25,
                        ["labels", "boxes", "cardinality"], "per level")
    H, W, N = 96, 160, 32
    with switches.override(FOD_ASYNC_MATCH="0"):
        for seed, counts in ((1, [5, 0, 17]), (2, [32, 1, 9])):
            logits, boxes, _ = _criterion_inputs(seed=seed, M=300)
            B = logits.shape[1]
            g = torch.Generator().manual_seed(seed)
            ab = torch.zeros(B, N, 4)
            x0 = torch.rand(B, N, generator=g) * (W - 20)
            y0 = torch.rand(B, N, generator=g) * (H - 20)
            ab[..., 0], ab[..., 1] = x0, y0
            ab[..., 2] = x0 + 4 + torch.rand(B, N, generator=g) * 15
            ab[..., 3] = y0 + 4 + torch.rand(B, N, generator=g) * 15
            cls = torch.randint(0, 8, (B, N), generator=g)
            act = torch.zeros(B, N, dtype=torch.int64)
            for b in range(B):
                act[b, torch.randperm(N, generator=g)[:counts[b]]] = 1
            targets = to_detr_targets(H=H, W=W, anno_active=act, anno_boxes=ab, anno_classes=cls)
            out_h = crit({"_stacked": (logits, boxes)}, targets, distributed=False)
            out_h.table[:, :3].sum().backward()
            ref = (out_h.table.detach().cpu(), logits.grad.clone().cpu(), boxes.grad.clone().cpu())
            logits.grad = None
            boxes.grad = None
            packed = ops.pack_targets_dev(ab.to(DEV), cls.to(DEV), act.to(DEV), H, W)
            assert packed["offset"].cpu().tolist() == [0] + list(np.cumsum(counts))
            nb = crit.device_num_boxes(packed["count"], distributed=False)
            out_d = crit({"_stacked": (logits, boxes)}, None, distributed=False, packed=packed, num_boxes=nb)
            out_d.table[:, :3].sum().backward()
            assert torch.equal(out_d.table.detach().cpu(), ref[0]), seed
            assert torch.equal(logits.grad.cpu(), ref[1]) and torch.equal(boxes.grad.cpu(), ref[2]), seed


# ---- the model ----------------------------------------------------------------------------------------------------
def _build(dtype, seed=3):
    """test_graph_gpu._build with 300 queries."""
    from types import SimpleNamespace
    from future_od.models.st_detr import SpatioTemporalDETRArgs
    from future_od.optim import FusedAdamW
    from oracle import stdetr as O
    from runs._model import build_model
    cfg = O.Config(backbone="resnet18", enc_layers=1, dec_layers=2, num_queries=300)
    args = SimpleNamespace(device=DEV, distributed=False, compute_dtype=dtype, backbone="resnet18")
    detr = SpatioTemporalDETRArgs(num_classes=8, num_queries=300, lr_backbone=1e-4, enc_layers=1, dec_layers=2,
                                  pretrained_backbone=False)
    model = build_model(args, detr)
    model.load_state_dict(O.make_state_dict(cfg, seed))
    model.eval()
    opt = FusedAdamW(model.parameters(), lr=1e-4, weight_decay=1e-4, max_norm=0.1)
    return model, opt


def _step(model, opt, data):
    opt.zero_grad()
    _, _, loss, stats, _ = model(data=data, distributed=False)
    loss.backward()
    opt.step()
    return float(loss.detach()), {k: v.detach().clone() for k, v in stats.items()}


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_eager_step_with_300_queries_device_matcher_against_host_matcher(dtype):
    from future_od.datasets.synthetic import make_batch
    from future_od.models.set_criterion import join_matchers
    data = make_batch(2, 3, 96, 128, seed=11, max_boxes=20, device=DEV)
    m_d, o_d = _build(dtype)
    m_h, o_h = _build(dtype)
    loss_d, stats_d = _step(m_d, o_d, data)
    join_matchers()                                                # the device solver's status word, now
    with switches.override(FOD_DEVICE_MATCH=0):
        loss_h, stats_h = _step(m_h, o_h, data)
        join_matchers()
    tol = 2e-5 if dtype == "fp32" else 2e-3
    assert np.isfinite(loss_d) and abs(loss_d - loss_h) <= tol * max(abs(loss_h), 1.0), (loss_d, loss_h)
    for k in ("class_error", "cardinality"):
        assert torch.equal(stats_d[k], stats_h[k]), (k, stats_d[k], stats_h[k])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_graphed_steps_with_300_queries_track_eager_steps(dtype):
    """test_graphed_steps_track_eager_steps on the 300-query model: one graph, its sequence, tolerances and bounds."""
    from future_od.datasets.synthetic import make_batch
    from future_od.graph import GraphedStep
    data = make_batch(2, 3, 96, 128, seed=11, max_boxes=9, device=DEV)
    data2 = make_batch(2, 3, 96, 128, seed=12, max_boxes=20, device=DEV)
    m_e, o_e = _build(dtype)
    m_g, o_g = _build(dtype)
    step = GraphedStep(m_g, o_g, warmup=2)
    seq = [data, data, data, data, data2, data, data2]
    le = [_step(m_e, o_e, d)[0] for d in seq]
    lg = [None, None, None, float(step(seq[3])[1].detach())]
    lg += [float(step(d)[1].detach()) for d in seq[4:]]
    assert step.replays == 4 and len(step._graphs) == 1
    assert o_g._step_no == o_e._step_no == len(seq)
    tol = 2e-5 if dtype == "fp32" else 2e-3
    for i in range(3, len(seq)):
        assert abs(lg[i] - le[i]) <= tol * max(abs(le[i]), 1.0), (i, lg[i], le[i])
    worst, total, count = 0.0, 0.0, 0
    for (_, pe), (_, pg) in zip(m_e.named_parameters(), m_g.named_parameters()):
        d = (pe.detach() - pg.detach()).abs()
        worst = max(worst, float(d.max()))
        total += float(d.sum())
        count += d.numel()
    if dtype == "fp32":
        assert worst < 3e-5, worst
    else:
        assert total / count < 2e-5 and worst < 1.5e-3, (total / count, worst)


def test_default_arguments_take_a_captured_training_step():
    """SpatioTemporalDETRArgs(num_classes=...) and nothing else (300 queries, six layers each way): one graph."""
    from types import SimpleNamespace
    from future_od.datasets.synthetic import make_batch
    from future_od.graph import GraphedStep
    from future_od.models.st_detr import SpatioTemporalDETRArgs
    from future_od.optim import FusedAdamW
    from runs._model import build_model
    detr = SpatioTemporalDETRArgs(num_classes=8)
    assert detr.num_queries == 300
    torch.manual_seed(0)
    model = build_model(SimpleNamespace(device=DEV, distributed=False, compute_dtype="bf16", backbone=detr.backbone), detr)
    model.eval()
    opt = FusedAdamW(model.parameters(), lr=1e-4, weight_decay=1e-4, max_norm=0.1)
    step = GraphedStep(model, opt, warmup=1)
    data = make_batch(2, 3, 96, 128, seed=11, max_boxes=20, device=DEV)
    losses = [float(step(data)[1].detach()) for _ in range(2)]
    assert len(step._graphs) == 1 and step.replays == 2 and all(np.isfinite(losses)), losses


def test_predict_with_300_queries_is_the_detector_of_forward_and_replays():
    from future_od.datasets.synthetic import make_batch
    from future_od.graph import GraphedPredict
    from test_predict_gpu import _same, _strip
    model, _ = _build("bf16")
    data = make_batch(2, 3, 96, 128, seed=11, max_boxes=20, device=DEV)
    with torch.no_grad():
        post = model(data=data, distributed=False)[0]
    cs, bp = post["class_scores"][:, 0, 0], post["boxes"][:, 0, 0]                   # [B,M,C+1], [B,M,4]
    assert cs.shape == (2, 300, 9)
    det = model.predict(data, top_k=100)
    assert det["count"].tolist() == [100, 100] and int(det["query"].max()) >= 256
    q, c = det["query"].long(), det["labels"].long()
    bi = torch.arange(2, device=DEV)[:, None]
    assert torch.equal(cs[bi, q, c], det["scores"]) and torch.equal(bp[bi, q], det["boxes"])
    free = _strip(data)
    gp = GraphedPredict(model, top_k=100)
    assert _same(gp(free), det) and _same(gp(free), model.predict(free, top_k=100))
    assert len(gp._graphs) == 1 and gp.replays == 2


# ---- launch shapes of a 300-query decoder ----------------------------------------------------------------------------
# (B, H, Tq, S, parts), blocks per 32-query tile, keys per block.  Two samples give 160 query tiles, so the keys are split
# over the four waves of a block only; one sample gives 80, and two blocks share a tile (last chunk 44 or 64 keys).
ATTN_300 = [((2, 8, 300, 300, 1), 1, 300), ((2, 8, 300, 320, 1), 1, 320), ((2, 8, 300, 320, 2), 1, 320),
            ((1, 8, 300, 300, 1), 2, 256), ((1, 8, 300, 320, 2), 2, 256)]


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("shape,ksplit,kchunk", ATTN_300, ids=["x".join(map(str, c[0])) for c in ATTN_300])
def test_attention_at_300_queries_takes_the_key_split(shape, ksplit, kchunk, dtype):
    """Tq = 300 with 300 or 320 keys, one and two parts: the few-query kernels that split the keys (Tq <= 512, with the
    scratch that S >= 256 asks for), forward and backward against float64 torch on the host with the bounds of
    tests/test_variants_gpu.py's attention cases."""
    import variant_cases as V
    from future_od.native import lib as L
    from test_variants_gpu import _attn_run_and_check
    r = ops.attn_route(*shape, V.DTYPE[dtype])
    assert (r.fwd, r.dq, r.key_split, r.ksplit, r.kchunk) == (L.ATTN_PLAIN, L.ATTN_PLAIN, 1, ksplit, kchunk)
    _attn_run_and_check(V.Case("attn_many_queries", {}, "attn", shape, dtype, {}, {}))


def test_fused_decoder_launches_on_600_rows():
    """B * M = 600 rows: a multiple of 8 but not of 16, 32 or 64, so the 16-row workgroups of fod_linear_add_norm_* and
    of the fod_mlp2_mul_* pair end ragged, and the grouped projections add a 300-row table.  The bodies (references and
    tolerances) are those of tests/test_kernels_gpu.py, run at these shapes."""
    import test_kernels_gpu as K
    K.test_fused_linear_add_norm_forward(600, True)
    K.test_fused_linear_add_norm_backward(600)
    K.test_fused_linear_add_norm_backward_pre(600, True)
    K.test_fused_mlp2_mul_forward_backward(2, 300)
    K.test_group_linear_with_per_segment_residual_tables(2, 300, 3, 2)
