"""The yardsticks recorded in tests/criterion_cases.py are what the measurement gives, and the cases satisfy what
tests/test_criterion_gpu.py assumes about them.  Everything here runs on the CPU from the same case builders; nothing
touches a device or the native library."""
import pytest
import torch

import criterion_cases as CC


def test_limits_are_the_stated_ones_or_three_times_a_recorded_measurement():
    assert CC.MEASURED_FACTOR == 3.0 and CC.COST_TOL == (2e-5, 1e-5)
    assert CC.LOSS_TOL == {"loss": (1e-5, 2e-5), "class_error": (1e-4, 1e-5), "dlogits": (1e-6, 1e-4), "dboxes": (1e-5, 1e-4)}
    for band, m in CC.COST_MEASURED.items():
        assert CC.cost_limit(band) == (max(2e-5, 3.0 * m), 1e-5)
    for op, m in CC.TRACKER_MEASURED.items():
        assert CC.tracker_limit(op) == 3.0 * m


@pytest.mark.parametrize("band", list(CC.COST_MEASURED))
def test_recorded_cost_distance_is_current(band):
    """Within a factor of two either way: the figure is a maximum over a few thousand entries and hangs on single roundings
    of the sigmoid, so another libm may move it a little; changed cases move it by more and have to be measured again."""
    now, recorded = CC.measure_cost_band(band), CC.COST_MEASURED[band]
    assert 0.5 * recorded <= now <= 2.0 * recorded, (band, now, recorded)


@pytest.mark.parametrize("op", list(CC.TRACKER_MEASURED))
def test_recorded_tracker_distance_is_current(op):
    now, recorded = CC.measure_tracker(op), CC.TRACKER_MEASURED[op]
    assert 0.5 * recorded <= now <= 2.0 * recorded, (op, now, recorded)


def test_the_cost_is_ill_conditioned_at_confident_logits():
    """Why the saturated band is not compared element by element: the float32 oracle itself is far from float64 there."""
    worst = 0.0
    for name in CC.COST_CASES:
        d = CC.build_cost_case(name, "saturated")
        worst = max(worst, float((CC.cost_reference(d, torch.float32).double() - CC.cost_reference(d)).abs().max()))
    assert worst > 1000 * CC.cost_limit("8")[0], worst


@pytest.mark.parametrize("name", list(CC.LOSS_CASES))
def test_float32_oracle_stays_within_the_loss_limits(name):
    """The limits applied to the kernels leave room for float32 itself; the builder asserts that matched rows have no tied
    top logits and that the per-sample counts are the stated ones."""
    d = CC.build_loss_case(name)
    ref = CC.loss_reference(d)
    assert all(bool(torch.isfinite(t).all()) for t in ref)
    CC.check_loss(CC.loss_reference(d, torch.float32), ref, name + ": ")
    c = d.case
    if c.M >= 8:                                   # one row exactly on the cardinality threshold, one just above it
        assert bool((d.logits[:, :, 0].amax(-1) == 0.5).all()) and bool((d.logits[:, :, 1].amax(-1) == CC.HALF_UP).all())
        assert CC.HALF_UP > 0.5
    if c.band == "saturated":
        assert {float(v) for v in CC.SATURATED_VALUES} <= set(d.logits[0, 0].flatten().tolist())


def test_case_table_covers_the_sizes_it_claims():
    cases = [c for n, c in CC.LOSS_CASES.items() if not n.startswith("pair_")]
    assert {1, 255, 256, 257, 300, 513} <= {c.M for c in cases}
    assert {1, 3} <= {c.B for c in cases} and {1, 3} <= {c.L for c in cases}
    assert {1, 3, 8, 10, 91} <= {c.C for c in cases}
    assert {0.25, 0.6} <= {c.alpha for c in cases} and {"moderate", "saturated"} == {c.band for c in cases}
    assert any(n in (0, 1) for c in cases for n in c.counts) and any(c.M in c.counts for c in cases)
    assert any(sum(c.counts) == 0 and c.B > 1 for c in cases)
    assert any(c.num_boxes is not None and c.num_boxes != int(c.num_boxes) for c in cases)
    assert any((c.B * c.M * c.C) % 256 for c in cases)
    cost = list(CC.COST_CASES.values())
    assert {(c.L * c.B * c.M) % 4 for c in cost} == {0, 1, 2, 3}
    assert {0, 1, 64, 65, 130} <= {n for c in cost for n in c.counts}
    assert {1, 10, 91} <= {c.C for c in cost} and {2.0, 1.5} == {c.gamma for c in cost} and {0.25, 0.6} == {c.alpha for c in cost}
    assert any(c.weights != (2.0, 5.0, 2.0) for c in cost)
    for name in CC.COST_CASES:
        d = CC.build_cost_case(name, "4")
        assert int(d.tl.max()) == d.case.C - 1


@pytest.mark.parametrize("pair", list(CC.GEOMETRY))
def test_dyadic_pairs_take_the_same_branch_in_float32_and_float64(pair):
    """Float32 autograd equals float64 autograd to 1e-6 on the hand-built pairs: no min / max / clamp decision flips."""
    d = CC.build_loss_case("pair_" + pair)
    a, b = CC.loss_reference(d, torch.float32), CC.loss_reference(d)
    assert float((a[2].double() - b[2]).abs().max()) <= 1e-6 and float((a[0][:, 1:3].double() - b[0][:, 1:3]).abs().max()) <= 1e-6
    pred, tgt = (torch.tensor(v, dtype=torch.float64) for v in CC.GEOMETRY[pair])
    assert bool((pred * 1024 == (pred * 1024).round()).all()) and bool((tgt * 1024 == (tgt * 1024).round()).all())


def test_touching_pair_has_the_gradient_quoted_in_the_design_notes():
    d = CC.build_loss_case("pair_touching_x")
    pred = d.boxes[0, 0, 0].double().requires_grad_(True)
    tgt = d.tb[0].double()
    loss = 1 - CC.tp.generalized_box_iou(CC.tp.box_cxcywh_to_xyxy(pred[None]), CC.tp.box_cxcywh_to_xyxy(tgt[None]))[0, 0]
    (grad,) = torch.autograd.grad(loss, pred)
    assert torch.allclose(grad, torch.tensor([-11 / 12, 0.0, -17 / 24, 0.5], dtype=torch.float64), atol=1e-12), grad


@pytest.mark.parametrize("name", list(CC.COST_CASES))
def test_float32_oracle_stays_within_the_cost_limits(name):
    for band in ("4", "8"):
        d = CC.build_cost_case(name, band)
        valid = CC.cost_valid(d).expand(d.case.L, -1, d.case.M, -1)
        ok, worst = CC.within(CC.cost_reference(d, torch.float32)[valid], CC.cost_reference(d)[valid], CC.cost_limit(band))
        assert ok, (name, band, worst)
    d = CC.build_cost_case(name, "saturated")
    f32 = CC.cost_reference(d, torch.float32)
    lo, hi = CC.cost_envelope(d, 0)
    assert torch.equal(lo, f32) and torch.equal(hi, f32)            # zero ulps: the envelope is the oracle itself
    assert CC.envelope_excess(f32, d) <= 0.0 and bool(torch.isfinite(f32).all())
    assert float(d.logits.abs().max()) == 30.0
