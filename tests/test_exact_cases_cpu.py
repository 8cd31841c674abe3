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


# ================================================================================================ the fused kernels
# tests/fused_exact_cases.py: the frozen bottleneck in one launch (three profiles, each with one dense stage) and the forward
# of the fused projection + add + norm.
import fused_exact_cases as FX                       # noqa: E402


def test_fused_table_ids_are_unique_and_the_thin_weights_are_gathers():
    ids = [FX.bnk_id(c) for c in FX.BNK_CASES] + [FX.lan_id(c) for c in FX.LAN_CASES]
    assert len(set(ids)) == len(ids) and not set(ids) & {E.case_id(c) for c in E.CASES}
    for cin in FX.CINS:
        w1 = FX.thin_w1(cin, 3)
        assert set(w1.unique().tolist()) == {-0.5, 0.0, 0.5} and bool(((w1 != 0).sum(1) == 1).all()) and bool(((w1 != 0).sum(0) <= 1).all())
        assert bool((w1 != 0).view(64, cin // 64, 64).any(2).any(0).all())                   # every 64-channel group of x is read
    w2, w3 = FX.thin_w2(4), FX.thin_w3(5)
    assert set(w2.unique().tolist()) == {0.0, 1.0} and bool((w2.sum((1, 2, 3)) == 1).all()) and bool((w2.sum((0, 1, 2)) == 1).all())
    assert bool((w2.sum((0, 3)) >= 7).all())                                                 # all nine tap positions, 7 or 8 times each
    assert set(w3.unique().tolist()) == {0.0, 1.0} and bool((w3.sum(1) == 1).all()) and bool((w3.sum(0) == 4).all())


def test_fused_census():
    """Per profile and Cin: 12 shapes on the persistent kernel ("4"), 9 on the one-tile-per-workgroup kernel ("2": the eight
    edge shapes and the ragged multi-tile shape) -- 21 cases, 126 in all; both shortcut forms; every purpose of the shape table."""
    from collections import Counter
    assert len(FX.BNK_CASES) == 126
    assert Counter((c.profile, c.cin, c.version) for c in FX.BNK_CASES) == {(p, cin, v): n for p in FX.PROFILES for cin in FX.CINS
                                                                            for v, n in (("4", 12), ("2", 9))}
    want_purposes = {"4": {"sub-tile": 5, "one-tile": 3, "seams": 1, "ragged": 1, "walk-2": 1, "walk-3": 1},
                     "2": {"sub-tile": 5, "one-tile": 3, "ragged": 1}}
    for p in FX.PROFILES:
        for cin in FX.CINS:
            for v in ("4", "2"):
                got = Counter(c.purpose for c in FX.BNK_CASES if (c.profile, c.cin, c.version) == (p, cin, v))
                assert got == want_purposes[v], (p, cin, v, got)
    for c in FX.BNK_CASES:
        o = FX.bnk_problem(c).ops if math.prod(c.shape) < FX.BIG else None
        if o is not None:
            assert (o["wd"] is None) == (c.cin == 256) and tuple(o["w2"].shape) == (64, 3, 3, 64) and o["x"].shape[-1] == c.cin
    # the tile counts the purposes rest on
    assert [FX.ntiles(s) for s in ((1, 6, 30), (1, 5, 29), (1, 7, 31), (1, 12, 60), (3, 1, 1))] == [1, 1, 4, 4, 3]
    # the persistent walk on the 256 compute units of the MI355X (the GPU test asserts it for the device it runs on)
    w2_, w3_ = FX.walk_of((3, 36, 450), 256), FX.walk_of((5, 37, 570), 256)
    assert (w2_["per"], w2_["busy"], w2_["grid"], w2_["last"]) == (2, 135, 256, 2)
    assert (w3_["per"], w3_["busy"], w3_["grid"], w3_["last"], w3_["mid_image"]) == (3, 222, 256, 2, True)
    assert len(FX.LAN_CASES) == 20 and Counter(c.M for c in FX.LAN_CASES) == {M: 4 for M in (1, 15, 16, 17, 100)}
    assert Counter((c.bias, c.then) for c in FX.LAN_CASES) == {(b, t): 5 for b in (False, True) for t in (False, True)}


@pytest.mark.parametrize("c", **FX.bnk_params(version="4"))
def test_fused_bottleneck_case_satisfies_the_preconditions(c):
    """Non-zero dense operands, partial sums below 2^24 units, Y1 and Y2 bf16 numbers before their rounding, |value before the
    last rounding| + 1 <= 256, every Y1 channel and tap position read where W2 is thin.  (The cases of kernel "2" share these
    problems.)  The magnitudes are statistical, not guaranteed (576 * 2 in s2): a seed that fails gets replaced in the table."""
    facts, st = FX.facts_and_stats(c.profile, c.cin, c.shape, c.seed)
    assert all(facts.values()), (facts, st)
    assert st["max_y1"] <= 256 and st["max_y2"] <= 256
    p = FX.bnk_problem(c)
    assert p.want.dtype == BF16 and tuple(p.want.shape) == c.shape + (256,) and float(p.want.min()) >= 0
    assert {(v2.profile, v2.cin, v2.shape, v2.seed) for v2 in FX.BNK_CASES if v2.version == "2"} <= \
        {(v4.profile, v4.cin, v4.shape, v4.seed) for v4 in FX.BNK_CASES if v4.version == "4"}


def test_fused_bottleneck_relu_cannot_hide_a_stage(capsys):
    """Clamp caps: pooled over a profile's problems at most 0.15 of the dense stage's outputs and at most 0.15 of the final
    outputs are clamped to 0, and no problem of 180 pixels or more exceeds 0.30.  Measured: dense stage 0.00004 (s1), 0.039
    (s2), 0.032 (s3); final outputs 0.006, 0.021, 0.032; the worst single problem of >= 180 pixels 0.061."""
    for profile in FX.PROFILES:
        tot = [0, 0, 0, 0]
        for cin in FX.CINS:
            for shape in FX.SHAPES:
                (c,) = [c for c in FX.BNK_CASES if (c.profile, c.cin, c.shape, c.version) == (profile, cin, shape, "4")]
                _, st = FX.facts_and_stats(profile, cin, shape, c.seed)
                for i, k in enumerate(("dense_clamped", "dense_numel", "out_clamped", "out_numel")):
                    tot[i] += st[k]
                if st["pixels"] >= 180:
                    assert st["dense_clamped"] <= 0.30 * st["dense_numel"] and st["out_clamped"] <= 0.30 * st["out_numel"], (profile, cin, shape, st)
        with capsys.disabled():
            print(f"\nclamped to 0, profile {profile}: dense stage {tot[0] / tot[1]:.5f}, final outputs {tot[2] / tot[3]:.5f}")
        assert tot[0] <= 0.15 * tot[1] and tot[2] <= 0.15 * tot[3], (profile, tot)


MUTANT_SHAPES = [(1, 12, 60), (2, 23, 41), (3, 1, 1)]


@pytest.mark.parametrize("shape", MUTANT_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("cin", FX.CINS)
@pytest.mark.parametrize("profile", FX.PROFILES)
def test_every_mutant_of_the_reference_changes_the_expected_output(profile, cin, shape):
    """Padding applied to x instead of Y1 (s2, s3), one product lost and one doubled in the profile's dense stage, the last
    column of a tile's Y2 taken from the next tile, bd dropped, a halo row read from the previous image where a tile range
    crosses images ((3, 1, 1)): each changes at least one element of the expected bf16 output in every profile it applies to."""
    p = FX.problem(profile, cin, shape)
    ms = FX.mutants(profile, cin, shape)
    assert {"lose_product", "double_product"} <= set(ms) and ("pad_x" in ms) == (profile != "s1") and ("no_bd" in ms) == (cin == 64)
    assert ("seam" in ms) == (shape != (3, 1, 1)) and ("wrong_image" in ms) == (shape == (3, 1, 1))
    assert torch.equal(FX.rounded(FX.forward(p.ops)), p.want)
    for name, m in ms.items():
        got = FX.rounded(FX.forward(p.ops, m))
        msg = E.mismatch(got, p.want, name)
        assert msg is not None, (profile, cin, shape, name)
        if name in ("lose_product", "double_product") and profile == "s1":      # one product of +-1 operands: one unit
            assert "max |got - want| 1.0" in msg, msg


# ---- what today's bound lets through.  The operands of test_fused_frozen_bottleneck_matches_the_layer_by_layer_path (its
# recipe on the CPU generator), the block emulated WITH the kernel's three roundings to bf16, defects put into the emulation,
# and that test's comparison: max |got - fp32 torch| <= 2e-2 * max |fp32 torch|.
GAUSS_SHAPE = (2, 23, 41)
GAUSS_PIXEL = (0, 8, 20)                       # the Y2 element that loses a product: this pixel, the channel largest there
# measured ratios max err / span (Cin 64 / Cin 256); the clean emulation is at 4.5e-3 / 4.0e-3:
#   pad_x 9.0e-2 / 3.4e-2, row_copy 2.0e-1 / 2.3e-1, lose_largest 2.7e-2 / 2.5e-2 (caught, barely),
#   lose_quartile 4.5e-3 / 4.0e-3: the figure does not move at all
ACCEPTED_TODAY = {"lose_quartile"}


def _gaussian_block(cin):
    from future_od.native import backbone as BB
    torch.manual_seed(5)
    blk = BB._Block("bottleneck", cin, 64, 1, 4)
    for m in blk.modules():
        if isinstance(m, BB.FrozenBatchNorm2d):
            m.weight.uniform_(0.5, 1.5); m.bias.normal_(0, 0.2); m.running_mean.normal_(0, 0.2); m.running_var.uniform_(0.5, 1.5)
    x = rnd(GAUSS_SHAPE + (cin,), BF16, 9)
    main, ds = blk.convs()
    o, names = dict(x=x, wd=None, bd=None), (("w1", "b1"), ("w2", "b2"), ("w3", "b3"), ("wd", "bd"))
    for (wn, bn_), (cw, bn) in zip(names, main + ([ds] if ds is not None else [])):
        scale, shift = bn.scale_shift()
        w = (cw.weight.detach() * scale.view(-1, 1, 1, 1)).to(BF16).permute(0, 2, 3, 1).contiguous()      # what prep_conv stores
        o[wn], o[bn_] = (w if wn == "w2" else w.view(w.shape[0], -1)), shift
    # fp32 torch on the unfolded weights, as the GPU test computes it
    def bnf(t, bn):
        sc, sh = bn.scale_shift()
        return t * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
    import torch.nn.functional as F
    xt = x.float().permute(0, 3, 1, 2)
    y = torch.relu(bnf(F.conv2d(xt, main[0][0].weight.float()), main[0][1]))
    y = torch.relu(bnf(F.conv2d(y, main[1][0].weight.float(), padding=1), main[1][1]))
    y = bnf(F.conv2d(y, main[2][0].weight.float()), main[2][1])
    sc_ = xt if ds is None else bnf(F.conv2d(xt, ds[0].weight.float()), ds[1])
    return o, torch.relu(y + sc_).permute(0, 2, 3, 1).detach()


@pytest.mark.parametrize("cin", FX.CINS)
def test_todays_bound_accepts_a_lost_product_in_the_fused_bottleneck_that_equality_rejects(cin, capsys):
    """On Gaussian operands the 2e-2-of-span bound of the existing test catches padding on the wrong tensor and a tile row
    copied from its neighbour; the largest-magnitude product of one Y2 element lost is caught with a margin of a quarter; the
    upper-quartile-magnitude product lost is ACCEPTED, the figure does not even move (the error stays below the roundings of
    the clean kernel).  Measured here with the bf16 roundings emulated, printed.  The exact comparison on the integer operands
    rejects the same defects."""
    o, ref = _gaussian_block(cin)
    bf16 = lambda t: t.to(F32).to(BF16).to(t.dtype)
    span = float(ref.abs().max())
    run = lambda m=None: FX.rounded(FX.forward(o, m, store=bf16)).float()
    ratio = lambda got: float((got - ref).abs().max()) / span
    clean = FX.forward(o, store=bf16)
    i, y, x_ = GAUSS_PIXEL
    c = int(clean.y2[i, y, x_].argmax())                                                  # (not one the relu clamps)
    y1p = torch.nn.functional.pad(clean.y1, (0, 0, 1, 1, 1, 1))
    terms = (o["w2"].double()[c] * y1p[i, y:y + 3, x_:x_ + 3]).abs().flatten()           # [ky, kx, k] -> 576 magnitudes
    order = terms.argsort()
    index = lambda flat: (i, y, x_, c, int(flat) // 192, int(flat) // 64 % 3, int(flat) % 64)
    mutants = {"pad_x": ("pad_x",), "row_copy": ("row_copy", 2, c), "lose_largest": ("lose_product", 2, index(order[-1])),
               "lose_quartile": ("lose_product", 2, index(order[len(order) * 3 // 4]))}
    base = run()
    assert ratio(base) <= 2e-2
    ratios = {}
    for name, m in mutants.items():
        got = run(m)
        assert not torch.equal(got, base), name
        ratios[name] = ratio(got)
    with capsys.disabled():
        print(f"\nfused bottleneck cin={cin} {GAUSS_SHAPE}: max err / span, clean {ratio(base):.2e}; "
              + ", ".join(f"{k} {v:.2e}" for k, v in ratios.items()) + "; today's bound 2e-2")
    assert {k for k, v in ratios.items() if v <= 2e-2} == ACCEPTED_TODAY, ratios
    # the integer counterpart: a lost product of the dense 3x3 (profile s2) changes the expected output
    p = FX.problem("s2", cin, GAUSS_SHAPE)
    assert E.is_exact(FX.rounded(FX.forward(p.ops)), p.want)
    for flat in (order[-1], order[len(order) * 3 // 4]):
        assert E.mismatch(FX.rounded(FX.forward(p.ops, ("lose_product", 2, index(flat)))), p.want, "lost product") is not None


@pytest.mark.parametrize("c", **FX.lan_params())
def test_fused_linear_add_norm_case_satisfies_the_preconditions(c):
    """The projection (rounded to bf16 by the kernel before x is added) and the sum are integers of at most 256 in magnitude
    with a margin of one, so both roundings change nothing; the mean is an exact f32 number."""
    p = FX.lan_problem(c.M, c.bias)
    for t in (p.proj, p.sum):
        assert bool((t == t.round()).all()) and float(t.abs().max()) + 1 <= 256
    assert all(bool((p.ops[k] != 0).all()) for k in ("a", "w")) and (p.ops["bias"] is None) == (not c.bias)
    assert torch.equal(p.want_sum.double(), p.sum) and torch.equal(p.want_mean.double(), p.sum.mean(-1))
    assert torch.equal(p.want_mean.double() * 256, p.sum.sum(-1))
