"""The table of exact-arithmetic cases (tests/exact_cases.py), the parts that need no GPU: every case satisfies the facts that
make equality the right comparison and takes the route the table says; the table as a whole reaches every NT / TN kernel,
tile, split and write mode of tests/variant_cases.py, every conv call and every epilogue combination; and, on the two
shapes the loose bound is weakest at, today's tolerance ACCEPTS a lost product, a dropped tail row and a pass through
bf16, which the exact comparison on the integer operands REJECTS."""
import math

import pytest
import torch

import exact_cases as E
import variant_cases as V
from future_od.native import lib as L
from test_kernels_gpu import check, rnd            # both import without a GPU (only `ops` / `lib` wait for one there)

BF16, F32 = torch.bfloat16, torch.float32


# ------------------------------------------------------------------------------------------------ the table
def test_table_ids_are_unique_and_the_recipes_hold_what_they_say():
    ids = [E.case_id(c) for c in E.CASES]
    assert len(set(ids)) == len(ids) and len(ids) >= 200
    assert set(E.pm1((4000,), 1).tolist()) == {-1.0, 1.0}
    assert set(E.nz3((4000,), 2).tolist()) == {-3.0, -2.0, -1.0, 1.0, 2.0, 3.0}
    assert set(E.col_scale(4000, 3).tolist()) == {-1.0, 1.0} and set(E.col_shift(4000, 4).tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert set(E.residual((4000,), 5, BF16).float().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert set(E.relu_mask((4000,), 6, BF16).float().tolist()) == {-1.0, 1.0}
    assert set(E.row_scale(4000, 7).tolist()) == {0.5, 1.0, 2.0}
    assert set(E.initial((4000,), 8).tolist()) == {float(v) for v in range(-4, 5)}
    assert torch.equal(E.nz3((5, 7), 9), E.nz3((5, 7), 9)) and not torch.equal(E.nz3((5, 7), 9), E.nz3((5, 7), 10))


@pytest.mark.parametrize("c", **E.params())
def test_case_satisfies_the_preconditions_and_takes_its_route(c):
    """No operand element that enters a product is zero, every sum of magnitudes is below 2^24, bf16 results and both their
    integer neighbours are bf16 numbers, row scales of 0.5 keep their margin; nothing is exempted.  The route the table
    records is the library's under the case's knobs and mode."""
    facts = E.preconditions(c)
    assert all(facts.values()), facts
    assert c.expect or c.call in ("colsum", "dilated", "stem", "stem_pool", "group", "group_res", "batched")
    assert V.route_mismatches(c.v) == []
    p = E.problem(c)
    for name, o in p.outs.items():
        want = E.expected(o)
        assert want.dtype == o.dtype and torch.equal(want.double(), o.pre), name          # the one rounding changes nothing


def test_variant_cases_are_all_taken_over():
    mine = {V.case_id(c.v) for c in E.CASES}
    for fam in ("nt128", "nt_splitk", "nt_big", "tn128", "tn_big"):
        for v in V.cases(fam):
            assert V.case_id(v) in mine or V.case_id(v._replace(extra=dict(v.extra, row_mod=True))) in mine, V.case_id(v)
    assert any(c.extra.get("det") for c in E.cases("tn128")) and any(c.extra.get("det") for c in E.cases("tn_big"))


def _values(cs, field):
    return {c.expect[field] for c in cs if field in c.expect}


def test_census():
    nt_calls, tn_calls = ("gemm_nt", "conv_fwd", "conv_dgrad"), ("gemm_tn", "conv_wgrad")
    nt_v = [v for v in V.CASES if v.call in nt_calls]
    tn_v = [v for v in V.CASES if v.call in tn_calls]
    nt_e = [c for c in E.CASES if c.call in nt_calls]
    tn_e = [c for c in E.CASES if c.call in tn_calls]
    # every NT kernel id, tile width, stage count, split count (and DMA interleave) of variant_cases has an exact case
    for field in ("kernel", "tile_n", "stages", "ksplit", "interleave"):
        assert _values(nt_v, field) and _values(nt_v, field) <= _values(nt_e, field), field
    assert _values(nt_e, "kernel") == {L.NT_128, L.NT_SMALL, L.NT_BIG}
    assert _values(nt_e, "ksplit") >= {1, 2, 3, 4, 8} and _values(nt_e, "tile_n") == {64, 128, 256}
    # ... every TN kernel id, tile family, workspace mode, block order; atomics (no workspace, not deterministic) and the
    # deterministic mode
    for field in ("kernel", "bi", "bj", "uses_partials_ws", "xcd_order", "nsplit"):
        assert _values(tn_v, field) and _values(tn_v, field) <= _values(tn_e, field), field
    assert _values(tn_e, "kernel") == {L.TN_128, L.TN_SMALL, L.TN_BIG}
    for kernel in (L.TN_128, L.TN_BIG):
        mine = [c for c in tn_e if c.expect.get("kernel") == kernel]
        assert {bool(c.extra.get("det")) for c in mine} == {False, True}
        atomics = [c for c in mine if not c.expect.get("uses_partials_ws") and not c.extra.get("det")]
        assert any(c.expect.get("nsplit", 1) > 1 for c in atomics)
        assert any(c.expect.get("uses_partials_ws") for c in mine)
    assert {(c.expect.get("bi"), c.expect.get("bj")) for c in tn_e if c.expect.get("kernel") == L.TN_BIG} >= {(256, 256), (None, None)}
    # every conv call in both dtypes: forward, input gradient with stride 1 and 2 and in place (stride-2 1x1), weight gradient
    for dt in V.BOTH:
        convs = [c for c in E.CASES if c.dtype == dt and c.call.startswith("conv_")]
        assert {c.call for c in convs} == {"conv_fwd", "conv_dgrad", "conv_wgrad"}
        dgrads = [c for c in convs if c.call == "conv_dgrad"]
        assert {c.shape[6] for c in dgrads} == {1, 2}
        in_place = [c for c in dgrads if "dgrad_in_place" in E.problem(c).outs]
        assert in_place and all(c.shape[5] == 1 and c.shape[6] == 2 for c in in_place)
        assert {c.call for c in E.CASES if c.dtype == dt} >= {"colsum", "dilated", "stem", "gemm_nt", "gemm_tn"}
    assert {c.call for c in E.CASES} >= {"stem_pool", "group", "group_res", "batched"}
    for kernel in (L.NT_128, L.NT_BIG):
        assert {c.call for c in nt_e if c.expect.get("kernel") == kernel} == set(nt_calls)
    # a_row_mod / residual_row_mod once per NT kernel (at least)
    assert {c.expect["kernel"] for c in nt_e if c.extra.get("row_mod")} == {L.NT_128, L.NT_SMALL, L.NT_BIG}
    # the epilogue sweep: each of the three NT kernels, all eight (residual, relu, mask) combinations with and without scale +
    # shift, for bf16 and for f32 output; full tiles and a ragged last m-tile; the scalar epilogue
    sweeps = [c for c in E.CASES if c.extra.get("sweep")]
    assert {c.expect["kernel"] for c in sweeps} == {L.NT_128, L.NT_SMALL, L.NT_BIG}
    assert any(c.shape == (150, 130, 64) and c.expect["kernel"] == L.NT_128 for c in sweeps)
    for c in sweeps:
        names = set(E.problem(c).outs)
        outs = (False, True) if c.dtype == "bf16" else (False,)
        assert names == {E.sweep_name(o, a, combo) for o in outs for a in (False, True) for combo in E.COMBOS}
        assert len(names) == 8 * 2 * len(outs)
        tile_m = 256 if c.expect["kernel"] == L.NT_BIG else 64 if c.expect["kernel"] == L.NT_SMALL else 128
        assert c.shape[0] > tile_m and c.shape[0] % tile_m                                  # full tiles and a ragged last one
    assert {o.dtype for c in sweeps if c.dtype == "bf16" for o in E.problem(c).outs.values()} == {BF16, F32}
    assert {c.dtype for c in sweeps if c.expect["kernel"] == L.NT_128} == {"bf16", "f32"}


# ------------------------------------------------------------------------------------------------ the comparison itself
def test_mismatch_report_names_the_count_the_first_index_the_range_and_the_difference():
    want = torch.arange(12.0).view(3, 4)
    assert E.mismatch(want.clone(), want) is None and E.is_exact(want.clone(), want)
    got = want.clone()
    got[1, 3] -= 2
    got[2, 3] -= 1
    msg = E.mismatch(got, want, "probe")
    assert "probe: 2/12 elements differ" in msg and "first at (1, 3): got 5.0, want 7.0, got - want = -2.0" in msg
    assert "rows 1..2 x columns 3..3 of [3, 4]" in msg
    assert E.mismatch(want.to(BF16), want) is not None and E.mismatch(want[:2], want) is not None       # dtype and shape count
    nan = want.clone()
    nan[0, 0] = float("nan")
    assert "1/12" in E.mismatch(nan, want)
    assert "elements 2..2 of 5" in E.mismatch(torch.tensor([0.0, 0, 1, 0, 0]), torch.zeros(5))


# ------------------------------------------------------------------------------------------------ the gap, demonstrated
# The corruptions, applied to a float64 result `ref` of `lhs^T-style` operands: what a masked-off last lane, a tail row
# dropped for one column, and partial results parked in bf16 would do.  `term(i, j, k)`: product k of output element (i, j).
def _lose_one_product(ref, term, depth):
    out = ref.clone()
    i, j = ref.shape[0] - 1, ref.shape[1] - 1
    out[i, j] -= term(i, j, depth - 1)
    return out


def _drop_last_reduction_row_of_last_column(ref, term, depth):
    out = ref.clone()
    j = ref.shape[1] - 1
    out[:, j] -= term(slice(None), j, depth - 1)
    return out


def _through_bf16(ref, term, depth):
    return ref.float().to(BF16).double()


CORRUPTIONS = {"one_product": _lose_one_product, "last_row_of_one_column": _drop_last_reduction_row_of_last_column,
               "through_bf16": _through_bf16}


def _accepted(got, want, dtype, scale):
    try:
        check(got, want, dtype, scale)
    except AssertionError:
        return False
    return True


TN_GAP, NT_GAP = (8200, 136, 72), (256, 256, 2048)
# What today's bound does catch at the seeds of the existing tests: the tail row dropped from a whole column of the NT result
# changes 256 elements by |a b| each, 23 of them by more than their bound of about 1.3 (the largest by 1.98).  The other five
# corruptions pass it.
CAUGHT_TODAY = {("nt", "last_row_of_one_column")}


@pytest.mark.parametrize("how", CORRUPTIONS)
def test_todays_bound_accepts_a_corrupted_weight_gradient_that_equality_rejects(how):
    """tn_big at (8200, 136, 72), bf16 operands, f32 result: the Gaussian inputs and the bound of
    test_tn_big_with_the_workspace_dense (check at the bf16 tolerance with atol scaled by sqrt(M))."""
    M, N1, K2 = TN_GAP
    assert [c for c in E.cases("tn_big", shape=TN_GAP, dtype="bf16")]
    g, x = rnd((M, N1), BF16, 1).double(), rnd((M, K2), BF16, 2).double()
    rs = (torch.rand(N1, generator=torch.Generator().manual_seed(3)) + 0.5).double()
    ref = (g.t() @ x) * rs[:, None]
    assert _accepted(ref.float(), ref, BF16, math.sqrt(M))
    bad = CORRUPTIONS[how](ref, lambda i, j, m: rs[i] * g[m, i] * x[m, j], M)
    assert not torch.equal(bad, ref)
    assert _accepted(bad.float(), ref, BF16, math.sqrt(M)) == (("tn", how) not in CAUGHT_TODAY)
    p = E.tn_problem(TN_GAP, "bf16", 1, True)
    o = p.outs["dw_zeroed"]
    gi, xi, ri = p.ops["g"].double(), p.ops["x"].double(), p.ops["rs"].double()
    want = E.expected(o)
    assert E.is_exact(o.pre.float(), want)
    bad = CORRUPTIONS[how](o.pre, lambda i, j, m: ri[i] * gi[m, i] * xi[m, j], M)
    assert E.mismatch(bad.float(), want, how) is not None


@pytest.mark.parametrize("how", CORRUPTIONS)
def test_todays_bound_accepts_a_corrupted_product_that_equality_rejects(how):
    """The short-launch NT kernel at (256, 256, 2048), bf16: the Gaussian inputs and the bounds of
    test_nt_short_launch_split_k.  A lost product and a dropped tail row are applied to the bf16 result (shift + residual),
    the pass through bf16 to the out_f32 result, which that test also holds to the bf16 bound."""
    M, N, K = NT_GAP
    assert [c for c in E.cases("nt_splitk", shape=NT_GAP)]
    a, b = rnd((M, K), BF16, 7).double(), rnd((N, K), BF16, 8).double()
    shift = torch.randn(N, generator=torch.Generator().manual_seed(3)).double()
    res = rnd((M, N), BF16, 9).double()
    prod = a @ b.t()
    p = E.nt_problem(NT_GAP, "bf16", 1)
    term = lambda i, j, k: a[i, k] * b[j, k]
    if how == "through_bf16":
        ref, o, ai, bi = prod.clamp(min=0), p.outs["relu_f32"], p.ops["a3"].double(), p.ops["b3"].double()
        bad = CORRUPTIONS[how](ref, term, K).float()
        assert _accepted(ref.float(), ref, BF16, math.sqrt(K))
    else:
        ref, o, ai, bi = prod + shift + res, p.outs["shift_res"], p.ops["a"].double(), p.ops["b"].double()
        bad = CORRUPTIONS[how](ref, term, K).float().to(BF16)
        assert _accepted(ref.float().to(BF16), ref, BF16, math.sqrt(K))
    assert not torch.equal(bad.double(), ref)
    assert _accepted(bad, ref, BF16, math.sqrt(K)) == (("nt", how) not in CAUGHT_TODAY)
    want = E.expected(o)
    assert E.is_exact(o.pre.float().to(o.dtype), want)
    bad = CORRUPTIONS[how](o.pre, lambda i, j, k: ai[i, k] * bi[j, k], K).float().to(o.dtype)
    assert E.mismatch(bad, want, how) is not None
