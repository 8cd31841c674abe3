"""fod_match_cost, fod_set_loss_fwd/bwd, fod_post_proc and fod_tracker_cost/extrapolate against float64 on the CPU, at the
sizes where their loops take another trip, at saturated logits and at boxes that touch, tie or coincide.  The cases, the
references and the limits are tests/criterion_cases.py; tests/test_criterion_limits_cpu.py checks that table without a GPU.
Every test prints the distance it measured before it asserts (pytest -s shows them)."""
import pytest
import torch

import criterion_cases as CC

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from future_od.native import ops

DEV = "cuda:0"


def _run_losses(d, num_boxes):
    args = [t.to(DEV) for t in (d.logits, d.boxes, d.match, d.tl, d.tb)]
    out = ops.set_loss_fwd(*args, d.toff.to(DEV), num_boxes, d.case.alpha)
    dl, db = ops.set_loss_bwd(*args, d.g.to(DEV), num_boxes, d.case.alpha)
    return out.cpu(), dl.cpu(), db.cpu()


@pytest.mark.parametrize("name", [n for n in CC.LOSS_CASES if not n.startswith("pair_")])
def test_set_losses_against_float64(name):
    """The five outputs per level and both gradients, once with `num_boxes` as a host float and once as a device scalar:
    each within the limits of the float64 reference, and the two runs equal bit for bit."""
    d = CC.build_loss_case(name)
    ref = CC.loss_reference(d)
    host = _run_losses(d, d.num_boxes)
    dev = _run_losses(d, torch.tensor([d.num_boxes], dtype=torch.float32, device=DEV))
    for what, got in (("host num_boxes ", host), ("device num_boxes ", dev)):
        assert all(bool(torch.isfinite(t).all()) for t in got), what
        print(name, what, [f"{CC.within(a, b, (0.0, 0.0))[1]:.2e}" for a, b in zip(got, ref)])
        CC.check_loss(got, ref, f"{name}, {what}")
    assert all(torch.equal(a, b) for a, b in zip(host, dev))
    if not sum(d.case.counts):
        assert d.num_boxes == 1.0 and bool((host[0][:, 4] == 100.0).all())


@pytest.mark.parametrize("pair", list(CC.GEOMETRY))
def test_box_pair_loss_and_gradient_follow_float64_autograd(pair):
    """One matched pair alone (M = 1, num_boxes = 1): its L1 and GIoU loss and d/d(cx, cy, w, h) of the predicted box.  At
    min / max ties autograd splits the gradient evenly, and a clamp passes it where its argument is exactly 0: the touching
    pairs need `raw >= 0` in giou_loss_grad."""
    d = CC.build_loss_case("pair_" + pair)
    ref = CC.loss_reference(d)
    got = _run_losses(d, d.num_boxes)
    print(pair, "loss", got[0][0, 1:3].tolist(), ref[0][0, 1:3].tolist(), "dbox", got[2].flatten().tolist(),
          ref[2].flatten().tolist())
    CC.check_loss(got, ref, pair + ": ")


@pytest.mark.parametrize("band", CC.COST_BANDS)
@pytest.mark.parametrize("name", list(CC.COST_CASES))
def test_match_cost_against_float64(name, band):
    d = CC.build_cost_case(name, band)
    c = d.case
    got = ops.match_cost(d.logits.to(DEV), d.boxes.to(DEV), d.tl.to(DEV), d.tb.to(DEV), d.toff.to(DEV), c.ld,
                         *c.weights, alpha=c.alpha, gamma=c.gamma).cpu()
    assert got.shape == (c.L, c.B, c.M, c.ld) and bool(torch.isfinite(got).all())
    valid = CC.cost_valid(d).expand_as(got)
    assert bool((got[~valid] == 0).all()), "columns at and beyond a sample's count hold the wrapper's zeros"
    ref = CC.cost_reference(d)
    if band == "saturated":
        # element-wise closeness to float64 means nothing here (COST_MEASURED's comment): the envelope instead
        excess = {k: CC.envelope_excess(got, d, k) for k in range(CC.SAT_ULPS + 1)}
        print(name, band, "outside the envelope of k ulps by", excess, "| max distance to float64",
              float((got.double() - ref)[valid].abs().max()))
        assert excess[CC.SAT_ULPS] <= 0.0, excess
    else:
        ok, worst = CC.within(got[valid], ref[valid], CC.cost_limit(band))
        print(name, band, "max distance to float64", float((got.double() - ref)[valid].abs().max()), "limit",
              CC.cost_limit(band))
        assert ok, (name, band, worst)


@pytest.mark.parametrize("R,C", CC.POST_PROC_CASES)
def test_post_proc_against_float64(R, C):
    g = torch.Generator().manual_seed(100 * R + C)
    logits = torch.randn(R, C, generator=g) * 4
    logits.view(-1)[::7] = 104.0                          # expf(104) overflows: the sigmoid is 0 there, 1 at +104
    logits.view(-1)[3::7] = -104.0
    boxes = torch.rand(R, 4, generator=g)
    s, bp = ops.post_proc(logits.to(DEV), boxes.to(DEV), 448, 800)
    sr = logits.double().sigmoid()
    want = torch.cat([sr, sr.max(1, keepdim=True)[0]], 1)
    bb = boxes.double() * torch.tensor([800.0, 448.0, 800.0, 448.0], dtype=torch.float64)
    want_b = torch.cat([bb[:, :2] - 0.5 * bb[:, 2:], bb[:, :2] + 0.5 * bb[:, 2:]], -1)
    print(R, C, "scores", float((s.cpu().double() - want).abs().max()), "boxes", float((bp.cpu().double() - want_b).abs().max()))
    assert s.shape == (R, C + 1) and bool(torch.isfinite(s).all())
    assert CC.within(s, want, (1e-6, 1e-5))[0]            # close() of tests/test_heads_gpu.py: atol as given, rtol 1e-5
    assert CC.within(bp, want_b, (1e-4, 1e-5))[0]


@pytest.mark.parametrize("name", list(CC.TRACKER_COST_CASES))
def test_tracker_cost_against_float64(name):
    d = CC.build_tracker_case(name, *CC.TRACKER_COST_CASES[name])
    got = ops.tracker_cost(d.b2.to(DEV), d.l2.to(DEV), d.b1.to(DEV), d.l1.to(DEV))
    err = CC.scaled_error(got, CC.tracker_cost_reference(d))
    print(name, "tracker_cost", err, "limit", CC.tracker_limit("cost"))
    assert err <= CC.tracker_limit("cost")


@pytest.mark.parametrize("with_factor", [False, True], ids=CC.TRACKER_FACTORS)
@pytest.mark.parametrize("mode", CC.TRACKER_MODES, ids=lambda m: str(m).lower())
def test_tracker_extrapolate_against_float64(mode, with_factor):
    """All four size modes, rows without a previous detection (-1), factors 0, -0.5 and 1.75 or none at all."""
    d = CC.build_tracker_case("extrapolate", *CC.TRACKER_EXTRAPOLATE_SHAPE)
    assert bool((d.mapping == -1).any()) and bool((d.mapping >= 0).any())
    boxes, logits = ops.tracker_extrapolate(d.b2.to(DEV), d.l2.to(DEV), d.b1.to(DEV), d.l1.to(DEV), d.mapping.to(DEV),
                                            d.factor.to(DEV) if with_factor else None, mode)
    rb, rl = CC.tracker_extrapolate_reference(d, mode, with_factor)
    op = "extrapolate_" + str(mode).lower()
    errs = CC.scaled_error(boxes, rb), CC.scaled_error(logits, rl)
    print(op, with_factor, errs, "limit", CC.tracker_limit(op))
    assert max(errs) <= CC.tracker_limit(op)
