"""The GEMM, convolution and stem kernels on operands for which their arithmetic is exact, compared for EQUALITY.

tests/test_kernels_gpu.py and tests/test_variants_gpu.py hold these kernels to atol = c * sqrt(reduction length) + rtol * |ref|
on Gaussian inputs: a wrong tile fails that, one lost or doubled product in one element, a tail row dropped for one column or
a partial result parked in bf16 does not (tests/test_exact_cases_cpu.py shows it on two shapes).  Here the operands are small
non-zero integers (tests/exact_cases.py): every product and every partial sum in an f32 accumulator is an exact integer in
any order, under any split and any interleaving of atomics, so each result must EQUAL the float64 reference rounded once to
the output dtype -- torch.equal on the full tensor, no tolerance, no element exempted.  Every case sets its knobs, asks the
library which kernel the call is about to take and holds that against the table before it runs.

At the end of the file: the fused bottleneck and the forward of the fused projection + add + norm, on the operand profiles
of tests/fused_exact_cases.py."""
import contextlib

import pytest
import torch

import exact_cases as E
import variant_cases as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

if torch.cuda.is_available():
    from future_od.native import functional as Fn
    from future_od.native import lib as L
    from future_od.native import ops


@pytest.fixture(autouse=True)
def _mode_is_restored():
    prev = ops.is_deterministic()
    yield
    ops.set_deterministic(prev)


@pytest.fixture
def knobs():
    """knobs(FOD_X=v, ...): sets selection knobs of the library (csrc/knobs.h) for the rest of the test; the values
    they had come back at teardown."""
    with contextlib.ExitStack() as stack:
        yield lambda **values: stack.enter_context(L.knobs(**values))


def _enter(knobs, c):
    """The case's knobs and mode for the rest of the test; the route of the call that follows, held against the table."""
    knobs(**c.knobs)
    ops.set_deterministic(bool(c.extra.get("det", False)))
    return V.assert_route(c.v)


def exact(got, out, what):
    """THE comparison of this file: `got` equals the reference, rounded once to the output dtype, bit for bit; the report
    (exact_cases.mismatch) says how many elements differ, where the first is, which rows and columns hold them all, and
    got - want there."""
    msg = E.mismatch(got, E.expected(out), what)
    assert msg is None, msg


def dev(t):
    return None if t is None else t.to(DEV)


def _runs(c):
    return 3 if c.extra.get("det") else 1


# ------------------------------------------------------------------------------------------------ gemm_nt
@pytest.mark.parametrize("c", **E.params(call="gemm_nt", sweep=None))
def test_gemm_nt_is_exact(knobs, c):
    """Every NT route: the plain product, shift + residual, relu with out_f32 (nz3 operands: the result is f32); a_row_mod and
    residual_row_mod once per kernel.  Split-K launches are issued twice on one stream (the second finds the tickets and the
    scratch the first left), both results are compared, and the tickets are zero afterwards."""
    r = _enter(knobs, c)
    p = E.problem(c)
    M = c.shape[0]
    o = {k: dev(t) for k, t in p.ops.items()}
    calls = 2 if r.ksplit > 1 else 1
    got = []
    for _ in range(calls):
        res = {"plain": ops.gemm_nt(o["a"], o["b"]),
               "shift_res": ops.gemm_nt(o["a"], o["b"], shift=o["shift"], residual=o["res"]),
               "relu_f32": ops.gemm_nt(o["a3"], o["b3"], relu=True, out_f32=True)}
        if c.extra.get("row_mod"):
            res["a_row_mod"] = ops.gemm_nt(o["a"][:E.ROW_MOD].contiguous(), o["b"], a_row_mod=E.ROW_MOD, m_rows=M)
            res["res_row_mod"] = ops.gemm_nt(o["a"], o["b"], residual=o["res_p"], residual_row_mod=E.ROW_MOD)
        got.append(res)
    for i, res in enumerate(got):
        assert set(res) == set(p.outs)
        for name, t in res.items():
            exact(t, p.outs[name], f"{E.case_id(c)} {name} call {i}")
    if r.ksplit > 1:
        tickets = ops._workspace(L.WS_NT_SPLIT_TICKETS, o["a"].device)
        assert int(tickets.abs().sum()) == 0, "split-K tickets were not left at zero"


@pytest.mark.parametrize("c", **E.params(call="gemm_nt", sweep=True))
def test_gemm_nt_epilogue_sweep_is_exact(knobs, c):
    """All eight (residual, relu, mask) combinations -- the six the vector epilogue specialises for full bf16 tiles and the
    two it leaves to the generic loop -- with scale + shift and with neither, rounded to bf16 and written as f32, on full
    tiles and the ragged last m-tile of each NT kernel; on (150, 130, 64) the scalar epilogue (N % 4 != 0)."""
    _enter(knobs, c)
    p = E.problem(c)
    o = {k: dev(t) for k, t in p.ops.items()}
    seen = set()
    for f32_out in ((False, True) if c.dtype == "bf16" else (False,)):
        a, b = (o["a3"], o["b3"]) if f32_out else (o["a"], o["b"])
        for affine in (False, True):
            for combo in E.COMBOS:
                has_res, relu, has_mask = combo
                name = E.sweep_name(f32_out, affine, combo)
                y = ops.gemm_nt(a, b, scale=o["scale"] if affine else None, shift=o["shift"] if affine else None,
                                residual=o["res"] if has_res else None, relu=relu, relu_mask=o["mask"] if has_mask else None,
                                out_f32=f32_out)
                exact(y, p.outs[name], f"{E.case_id(c)} {name}")
                seen.add(name)
    assert seen == set(p.outs)


# ------------------------------------------------------------------------------------------------ gemm_tn_acc, colsum_acc
@pytest.mark.parametrize("c", **E.params(call="gemm_tn"))
def test_gemm_tn_acc_is_exact(knobs, c):
    """Every TN route -- the short reduction, both block orders, forced rows per split, partial tiles in the workspace and
    f32 atomics, both big tile families -- with row scales from {0.5, 1, 2} and fused column sums, into zeroed and into
    non-zero buffers.  Atomics are exact on integers: the non-deterministic routes equal the reference bit for bit as well;
    in deterministic mode three runs are compared."""
    _enter(knobs, c)
    p = E.problem(c)
    g, x, rs = dev(p.ops["g"]), dev(p.ops["x"]), dev(p.ops.get("rs"))
    assert (rs is not None) == bool(c.extra.get("row_scale")) and c.extra.get("colsum")
    for zeroed in (False, True):
        tag = "zeroed" if zeroed else "acc"
        for with_colsum in ((True, False) if rs is None else (True,)):          # the short reduction also without the fused sums
            for i in range(_runs(c)):
                dw = (torch.zeros_like(p.ops["dw0"]) if zeroed else p.ops["dw0"]).clone().to(DEV)
                cs = (torch.zeros_like(p.ops["cs0"]) if zeroed else p.ops["cs0"]).clone().to(DEV)
                ops.gemm_tn_acc(g, x, dw, row_scale=rs, colsum=cs if with_colsum else None, zeroed=zeroed)
                exact(dw, p.outs["dw_" + tag], f"{E.case_id(c)} dw {tag} colsum={with_colsum} run {i}")
                if with_colsum:
                    exact(cs, p.outs["cs_" + tag], f"{E.case_id(c)} colsum {tag} run {i}")


@pytest.mark.parametrize("det", [False, True], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("c", **E.params(call="colsum"))
def test_colsum_acc_is_exact(c, det):
    ops.set_deterministic(det)
    p = E.problem(c)
    g = dev(p.ops["g"])
    M = c.shape[0]
    out = p.ops["out0"].clone().to(DEV)
    ops.colsum_acc(g, out)
    exact(out, p.outs["colsum"], f"{E.case_id(c)} colsum")
    if "grouped" in p.outs:
        grp = p.ops["grp0"].clone().to(DEV)
        ops.colsum_acc(g, grp, group_rows=M // 4)
        exact(grp, p.outs["grouped"], f"{E.case_id(c)} grouped colsum")


# ------------------------------------------------------------------------------------------------ convolutions
@pytest.mark.parametrize("c", **E.params(call="conv_fwd"))
def test_conv2d_fwd_is_exact(knobs, c):
    _enter(knobs, c)
    p = E.problem(c)
    o = {k: dev(t) for k, t in p.ops.items()}
    y = ops.conv2d_fwd(o["x"], o["w"], V.conv_geom(c.shape), scale=o["scale"], shift=o["shift"], residual=o["res"], relu=True)
    exact(y, p.outs["fwd"], f"{E.case_id(c)} fwd")


@pytest.mark.parametrize("c", **E.params(call="conv_dgrad"))
def test_conv2d_dgrad_is_exact(knobs, c):
    """Residual + mask; the in-place form of the stride-2 1x1 convolution (the backbone's shortcut), after which the pixels
    that no tap reaches still hold what the caller's buffer held."""
    _enter(knobs, c)
    p = E.problem(c)
    o = {k: dev(t) for k, t in p.ops.items()}
    geom = V.conv_geom(c.shape)
    dx = ops.conv2d_dgrad(o["dy"], o["w_t"], geom, residual=o["dres"], relu_mask=o["mask"])
    exact(dx, p.outs["dgrad"], f"{E.case_id(c)} dgrad")
    if "dgrad_in_place" in p.outs:
        pre = p.ops["pre"]
        buf = pre.clone().to(DEV)
        got = ops.conv2d_dgrad(o["dy"], o["w_t"], geom, residual=buf, relu_mask=o["mask"], out=buf)
        assert got.data_ptr() == buf.data_ptr()
        exact(buf, p.outs["dgrad_in_place"], f"{E.case_id(c)} dgrad in place")
        back = buf.cpu()
        untouched = torch.equal(back[:, 1::2], pre[:, 1::2]) and torch.equal(back[:, :, 1::2], pre[:, :, 1::2])
        assert untouched, "pixels without taps were rewritten"


@pytest.mark.parametrize("c", **E.params(call="conv_wgrad"))
def test_conv2d_wgrad_acc_is_exact(knobs, c):
    _enter(knobs, c)
    p = E.problem(c)
    dy, x, rs = dev(p.ops["dy"]), dev(p.ops["x"]), dev(p.ops["rs"])
    geom = V.conv_geom(c.shape)
    for zeroed in (False, True):
        tag = "zeroed" if zeroed else "acc"
        for i in range(_runs(c)):
            dw = (torch.zeros_like(p.ops["dw0"]) if zeroed else p.ops["dw0"]).clone().to(DEV)
            ops.conv2d_wgrad_acc(dy, x, dw, geom, row_scale=rs, zeroed=zeroed)
            exact(dw, p.outs["dw_" + tag], f"{E.case_id(c)} dw {tag} run {i}")


@pytest.mark.parametrize("c", **E.params(call="dilated"))
def test_same_padded_dilated_conv_is_exact_with_its_gradients(c):
    """functional.conv2d_same(relu=True, dilation=d) through autograd: d * d convolutions on the parity sub-grids, their input,
    weight and bias gradients summed by autograd."""
    n, h, w_, cin, cout, k, d = c.shape
    p = E.problem(c)
    Fn.PREP.clear()
    x = dev(p.ops["x"]).requires_grad_(True)
    wg = torch.nn.Parameter(p.ops["wt"].contiguous(memory_format=torch.channels_last).to(DEV))
    bg = torch.nn.Parameter(dev(p.ops["b"]))
    y = Fn.conv2d_same(x, wg, bg, relu=True, dilation=d)
    y.backward(dev(p.ops["dy"]))
    for name, t in (("y", y), ("dx", x.grad), ("dw", wg.grad), ("db", bg.grad)):
        exact(t, p.outs[name], f"{E.case_id(c)} {name}")


# ------------------------------------------------------------------------------------------------ grouped and batched forms
@pytest.mark.parametrize("c", **E.params(call="group"))
def test_group_linear_kernels_are_exact(c):
    rows, D, K, P = c.shape
    p = E.problem(c)
    o = {k: dev(t) for k, t in p.ops.items()}
    exact(ops.group_linear_fwd(o["x"], o["w"], o["b"], P), p.outs["fwd"], f"{E.case_id(c)} fwd")
    exact(ops.group_linear_dgrad(o["g"], o["wt"], P), p.outs["dgrad"], f"{E.case_id(c)} dgrad")
    for zeroed in (False, True):
        tag = "zeroed" if zeroed else "acc"
        dw = (torch.zeros_like(p.ops["dw0"]) if zeroed else p.ops["dw0"]).clone().to(DEV)
        db = (torch.zeros_like(p.ops["db0"]) if zeroed else p.ops["db0"]).clone().to(DEV)
        ops.group_linear_wgrad(o["g3"], o["x3"], dw, db, zeroed=zeroed)
        exact(dw, p.outs["dw_" + tag], f"{E.case_id(c)} wgrad {tag}")
        exact(db, p.outs["db_" + tag], f"{E.case_id(c)} bias grad {tag}")


@pytest.mark.parametrize("c", **E.params(call="group_res"))
def test_group_linear_with_the_residual_table_is_exact(c):
    B, M, P, S = c.shape
    p = E.problem(c)
    o = {k: dev(t) for k, t in p.ops.items()}
    y = ops.group_linear_fwd(o["x"], o["w"], o["b"], P, residual=o["tables"], res_row_mod=M)
    exact(y, p.outs["fwd_res"], f"{E.case_id(c)} fwd with residual tables")


@pytest.mark.parametrize("c", **E.params(call="batched"))
def test_gemm_nt_batched_is_exact(c):
    P, M, N, K = c.shape
    p = E.problem(c)
    o = {k: dev(t) for k, t in p.ops.items()}
    exact(ops.gemm_nt_batched(o["a"], o["w"]), p.outs["plain"], f"{E.case_id(c)} plain")
    exact(ops.gemm_nt_batched(o["a"], o["w"], shift=o["bias"], relu=True), p.outs["shift_relu"], f"{E.case_id(c)} shift relu")
    exact(ops.gemm_nt_batched(o["a"], o["w"], shift=o["bias"], residual=o["res"], relu_mask=o["gate"]), p.outs["res_mask"],
          f"{E.case_id(c)} shift residual mask")
    exact(ops.gemm_nt_batched(o["a"], o["wt"], b_cols=True), p.outs["b_cols"], f"{E.case_id(c)} b_cols")


# ------------------------------------------------------------------------------------------------ stem
@pytest.mark.parametrize("c", **E.params_of(E.cases(call="stem") + E.cases(call="stem_pool")))
def test_stem_layout_conv_and_pool_are_exact(c):
    """clip_to_stem_layout on integer pixels, prep_stem with +-1 weights times a +-1 scale, conv_stem_fwd with an integer shift
    and relu = F.conv2d; stem_pool_fwd = F.max_pool2d of that, and equal to the two launches."""
    b, l, h, w_ = c.shape
    dtype = E.DTYPE[c.dtype]
    p = E.problem(c)
    Fn.PREP.clear()
    xp = ops.clip_to_stem_layout(dev(p.ops["video"]), dtype)
    exact(xp, p.outs["layout"], f"{E.case_id(c)} layout")
    weight = torch.nn.Parameter(p.ops["weight"].contiguous(memory_format=torch.channels_last).to(DEV))
    wprep = Fn.prep_stem(weight, dtype, dev(p.ops["scale"]).repeat_interleave(7).contiguous())
    shift = dev(p.ops["shift"])
    y = ops.conv_stem_fwd(xp, wprep, h, w_, shift=shift, relu=True)
    exact(y, p.outs["stem"], f"{E.case_id(c)} stem conv")
    if "pool" in p.outs:
        one = ops.stem_pool_fwd(xp, wprep, h, w_, shift=shift)
        exact(one, p.outs["pool"], f"{E.case_id(c)} stem + pool")
        exact(ops.maxpool3x3s2(y), p.outs["pool"], f"{E.case_id(c)} max-pool of the stem")


# ------------------------------------------------------------------------------------------------ the comparison bites
def test_one_flipped_operand_element_changes_exactly_its_products(knobs):
    """End to end through the real kernels, on the two shapes of the demonstration in tests/test_exact_cases_cpu.py: the sign
    of ONE operand element flipped on the device -- one product per output element of its row wrong by 2 |a b| -- and the
    comparison reports exactly that row, every column of it, and nothing else; the result still equals the reference of
    the flipped operands."""
    (c,) = [c for c in E.cases("nt_splitk", shape=(256, 256, 2048)) if not c.knobs]
    _enter(knobs, c)
    p = E.problem(c)
    M, N, K = c.shape
    a, b = p.ops["a"].clone(), p.ops["b"]
    a[M - 1, K - 1] = -a[M - 1, K - 1]
    got = ops.gemm_nt(a.to(DEV), b.to(DEV))
    msg = E.mismatch(got, E.expected(p.outs["plain"]), "flipped a")
    assert msg is not None and f"{N}/{M * N} elements differ" in msg and f"rows {M - 1}..{M - 1} x columns 0..{N - 1}" in msg, msg
    exact(got, p.outs["plain"]._replace(pre=a.double() @ b.double().t()), "the product of the flipped operand")

    (c,) = [c for c in E.cases("tn_big", shape=(8200, 136, 72)) if c.expect["uses_partials_ws"] and not c.extra.get("det")]
    _enter(knobs, c)
    p = E.problem(c)
    M, N1, K2 = c.shape
    g, x, rs = p.ops["g"].clone(), p.ops["x"], p.ops["rs"]
    g[M - 1, N1 - 1] = -g[M - 1, N1 - 1]
    dw = torch.zeros(N1, K2, device=DEV)
    ops.gemm_tn_acc(g.to(DEV), x.to(DEV), dw, row_scale=rs.to(DEV), zeroed=True)
    msg = E.mismatch(dw, E.expected(p.outs["dw_zeroed"]), "flipped g")
    assert msg is not None and f"{K2}/{N1 * K2} elements differ" in msg and f"rows {N1 - 1}..{N1 - 1} x columns 0..{K2 - 1}" in msg, msg
    exact(dw, p.outs["dw_zeroed"]._replace(pre=(g.double().t() @ x.double()) * rs.double()[:, None]), "the gradient of the flipped operand")


# ================================================================================================ the fused kernels
# tests/fused_exact_cases.py: three operand profiles, each with ONE dense stage and two thin ones (signed gathers), for which
# the two bf16 intermediates of the fused bottleneck are bf16 numbers before their rounding -- the whole block must EQUAL the
# float64 reference rounded once.  test_fused_frozen_bottleneck_matches_the_layer_by_layer_path (Gaussian magnitudes, the BN
# folding, 2e-2 of the span) stays as it is; tests/test_exact_cases_cpu.py shows what that bound lets through.
import fused_exact_cases as FX                       # noqa: E402

SENTINEL = -7.0                                      # no output of a block that ends in a relu


def _bnk_launch(o, shape):
    """ops.bottleneck_fused_fwd into the middle of a larger buffer: (result, buffer); guard images of the sentinel around it."""
    n, h, w = shape
    buf = torch.full((n + 2, h, w, 256), SENTINEL, dtype=torch.bfloat16, device=DEV)
    got = ops.bottleneck_fused_fwd(o["x"], o["w1"], o["b1"], o["w2"], o["b2"], o["w3"], o["b3"], o["wd"], o["bd"], out=buf[1:-1])
    assert got.data_ptr() == buf[1].data_ptr()
    return got, buf


def _guards_intact(buf, what):
    guards = torch.stack((buf[0], buf[-1])).cpu()
    assert bool((guards == SENTINEL).all()), f"{what}: {int((guards != SENTINEL).sum())} elements of the guard images were written"


def test_the_exact_bottleneck_weights_are_in_the_layout_prep_conv_produces():
    """[Cout][kh][kw][Cin]: prep_conv (no scale) of the OIHW channels_last parameter that holds the same taps gives the tensor
    the exact cases hand to the kernel."""
    o = FX.problem("s2", 64, (1, 1, 1)).ops
    Fn.PREP.clear()
    for name in ("w1", "w2", "w3", "wd"):
        w = o[name].float().view(o[name].shape[0], *((3, 3) if name == "w2" else (1, 1)), -1)          # [Cout, kh, kw, Cin]
        oihw = torch.nn.Parameter(w.permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last).to(DEV))
        prep = Fn.prep_conv(oihw, torch.bfloat16, None, False)
        assert torch.equal(prep.cpu().reshape(o[name].shape), o[name]), name


@pytest.mark.parametrize("c", **FX.bnk_params())
def test_fused_bottleneck_is_exact(knobs, c):
    """Both kernels of csrc/bottleneck_fused.hip, both shortcut forms, the integer weights and shifts handed to
    ops.bottleneck_fused_fwd directly (FrozenBatchNorm2d's rsqrt(var + eps) scale is not exactly 1): torch.equal on the full
    tensor; the guard images around the output are untouched (partial tiles must not store past the image).  On the
    persistent-walk shapes the device's CU count must give the walk the table intends (tiles per workgroup, a short last
    range, ranges that start mid-image), and a second launch on the same stream -- it meets the LDS and the ring as the first
    left them -- is compared too."""
    knobs(FOD_BNK_VERSION=c.version)
    p = FX.bnk_problem(c)
    o = {k: dev(t) for k, t in p.ops.items()}
    walk = FX.WALK.get(c.purpose)
    if walk:
        assert c.version == "4"
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        w = FX.walk_of(c.shape, cus)
        assert w["per"] == walk["per"] and w["busy"] <= w["grid"] == cus, (cus, w)
        if walk["short_last"]:
            assert 0 < w["last"] < w["per"] and w["mid_image"], (cus, w)
        else:
            assert w["busy"] < w["grid"], (cus, w)               # workgroups that find no tiles and leave at once
    runs = [_bnk_launch(o, c.shape) for _ in range(2 if walk else 1)]
    for i, (got, buf) in enumerate(runs):
        msg = E.mismatch(got, p.want, f"{FX.bnk_id(c)} launch {i}")
        assert msg is None, msg
        _guards_intact(buf, FX.bnk_id(c))


@pytest.mark.parametrize("cin", FX.CINS)
def test_fused_bottleneck_one_flipped_input_changes_exactly_its_outputs(knobs, cin):
    """(1, 12, 60), the dense 3x3 (s2): the sign of ONE x element flipped at pixel (5, 29), the corner four tiles share.  The
    result equals the reference of the flipped input, and the set of output elements that changed on the device is the
    reference's: the 3 x 3 neighbourhood through all three stages, nothing else -- a halo that a neighbouring tile read stale,
    or a tile that did not read it again, shows here."""
    knobs(FOD_BNK_VERSION="4")
    shape = (1, 12, 60)
    p = FX.problem("s2", cin, shape)
    k = int(p.ops["w1"].float()[0].abs().argmax())               # the input channel conv1's output channel 0 reads
    flipped = dict(p.ops, x=p.ops["x"].clone())
    flipped["x"][0, 5, 29, k] = -flipped["x"][0, 5, 29, k]
    want_f = FX.rounded(FX.forward(flipped))
    want_changed = want_f != p.want
    where = want_changed.any(-1)[0].nonzero()
    assert {tuple(t) for t in where.tolist()} == {(y, x) for y in (4, 5, 6) for x in (28, 29, 30)}        # all four tiles
    base, buf0 = _bnk_launch({n: dev(t) for n, t in p.ops.items()}, shape)
    got, buf1 = _bnk_launch({n: dev(t) for n, t in flipped.items()}, shape)
    for t, want, what in ((base, p.want, "as in the table"), (got, want_f, "one x element flipped")):
        msg = E.mismatch(t, want, f"bnk-s2-cin{cin} {what}")
        assert msg is None, msg
    assert torch.equal((got != base).cpu(), want_changed)
    _guards_intact(buf0, "base"), _guards_intact(buf1, "flipped")


@pytest.mark.parametrize("c", **FX.lan_params())
def test_fused_linear_add_norm_sum_and_mean_are_exact(c):
    """fod_linear_add_norm_fwd on +-1 operands with integer bias and x: the stored sum EQUALS a w^T + bias + x rounded once to
    bf16, the row mean -- (a sum of 256 integers) * 2^-8 -- equals the float64 mean bit for bit; ragged first and last groups
    of sixteen rows, with and without bias, plain and THEN form.  rstd, y and the THEN projection are not exact (rsqrt, Gaussian
    gamma / beta / weights): they keep the bounds of test_fused_linear_add_norm_forward and
    test_fused_linear_add_norm_then_next_projection, against the exact sum."""
    import torch.nn.functional as F
    from test_kernels_gpu import check
    p = FX.lan_problem(c.M, c.bias)
    o = {k: dev(t) for k, t in p.ops.items()}
    res = ops.linear_add_norm_fwd(o["a"], o["w"], o["bias"], o["x"], o["gamma"], o["beta"],
                                  **(dict(then_w=o["then_w"], then_bias=o["then_b"]) if c.then else {}))
    y, s, mean, rstd = res[:4]
    msg = E.mismatch(s, p.want_sum, f"{FX.lan_id(c)} sum")
    assert msg is None, msg
    msg = E.mismatch(mean, p.want_mean, f"{FX.lan_id(c)} mean")
    assert msg is None, msg
    assert torch.allclose(rstd.cpu(), (p.sum.var(-1, unbiased=False) + 1e-5).rsqrt().float(), rtol=1e-4)
    ref = F.layer_norm(p.sum, (256,), p.ops["gamma"].double(), p.ops["beta"].double(), 1e-5)
    check(y, ref.float(), torch.bfloat16, 4, FX.lan_id(c))
    if c.then:
        q_ref = ops.gemm_nt(y, o["then_w"], shift=o["then_b"])
        assert float((res[4].float() - q_ref.float()).abs().max()) <= 2.0 ** -7 * float(q_ref.float().abs().max())
