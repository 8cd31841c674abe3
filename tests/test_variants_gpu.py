"""Every selectable kernel variant against a high-precision torch computation of the same operation.

tests/test_kernels_gpu.py is thorough for the variant the default rule picks at small shapes; the siblings -- the other
tile width, split counts, block orders, ring depths, fallback kernels -- are reached here through the knobs of
csrc/knobs.h, at the smallest shapes at which each edge exists.  The cases live in tests/variant_cases.py (their routes
are verified without a GPU by tests/test_dispatch_cpu.py); every test below sets the case's knobs, ASKS the library
which kernel the call is about to take and compares that with the table, then compares every element of every result
with a float64 reference computed from the same (rounded) inputs.  Tolerances: check() / tol() of test_kernels_gpu.py
(f32 2e-5, bf16 2 ulp, atol scaled by the square root of the reduction length); attention and fp8 keep the bounds of
their tests there.  FOD_LN_BWD_GROUPS and FOD_FP8_STAGE have no route query: those two are only read back."""
import contextlib
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import variant_cases as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

if torch.cuda.is_available():
    from future_od.native import lib as L
    from future_od.native import ops
    from test_kernels_gpu import (_attn_ref, _conv_ref, _drop_keep_mask, attention_fp8_forward_and_backward, check,
                                  deferred_max_and_extreme_scores, rnd, saturated_softmax_forward_backward)


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
    return V.assert_route(c)


def _params(family, **where):
    cs = V.cases(family, **where)
    return dict(argvalues=cs, ids=[V.case_id(c) for c in cs])


def _out_dtype(dtype):
    return torch.float32 if dtype == torch.float32 else dtype


# ------------------------------------------------------------------------------------------------ NT, 128-wide tile
@pytest.mark.parametrize("c", **_params("nt128", call="gemm_nt", full_epilogue=None))
def test_nt128_wide_tile_dense(knobs, c):
    """Ragged last N tile, one row, N % 4 != 0 (the scalar epilogue), with and without an epilogue."""
    _enter(knobs, c)
    dtype = V.DTYPE[c.dtype]
    M, N, K = c.shape
    a, b = rnd((M, K), dtype, 1), rnd((N, K), dtype, 2)
    acc = a.double() @ b.double().t()
    check(ops.gemm_nt(a.to(DEV), b.to(DEV)), acc, dtype, math.sqrt(K), f"nt128 {c.shape}")
    scale, shift, res = torch.rand(N) + 0.5, torch.randn(N), rnd((M, N), dtype, 3)
    out = ops.gemm_nt(a.to(DEV), b.to(DEV), scale=scale.to(DEV), shift=shift.to(DEV), residual=res.to(DEV), relu=True)
    ref = (acc * scale.double() + shift.double() + res.double()).clamp(min=0)
    check(out, ref, dtype, math.sqrt(K), f"nt128 {c.shape} scale shift residual relu")


@pytest.mark.parametrize("c", **_params("nt128", full_epilogue=True))
def test_nt128_wide_tile_epilogues(knobs, c):
    """The epilogue set of test_gemm_nt_epilogue on the 128-wide tile."""
    _enter(knobs, c)
    dtype = V.DTYPE[c.dtype]
    M, N, K = c.shape
    a, b = rnd((M, K), dtype, 1), rnd((N, K), dtype, 2)
    scale, shift = torch.rand(N) + 0.5, torch.randn(N)
    res = rnd((50, N), dtype, 3)
    mask = rnd((M, N), dtype, 4)
    prod = a.double() @ b.double().t()
    acc = prod * scale.double() + shift.double() + res.double().repeat(3, 1)
    ref = torch.where(mask.double() > 0, acc.clamp(min=0), torch.zeros((), dtype=torch.float64))
    out = ops.gemm_nt(a.to(DEV), b.to(DEV), scale=scale.to(DEV), shift=shift.to(DEV), residual=res.to(DEV),
                      residual_row_mod=50, relu=True, relu_mask=mask.to(DEV))
    check(out, ref, dtype, 8, "epilogue")
    out32 = ops.gemm_nt(a.to(DEV), b.to(DEV), shift=shift.to(DEV), out_f32=True)
    assert out32.dtype == torch.float32
    check(out32, prod + shift.double(), _out_dtype(dtype), 8, "out_f32")
    out = ops.gemm_nt(a[:50].contiguous().to(DEV), b.to(DEV), a_row_mod=50, m_rows=M)
    check(out, (a[:50].double() @ b.double().t()).repeat(3, 1), dtype, 8, "a_row_mod")


def _conv_inputs(shape, dtype):
    n, h, w_, cin, cout, k, stride, pad = shape
    x = rnd((n, h, w_, cin), dtype, 1)
    w = rnd((cout, k, k, cin), dtype, 2, scale=1.0 / math.sqrt(k * k * cin))
    geom = ops.conv_geom(x.shape, cout, k, stride, pad)
    x64 = x.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    y_lin = F.conv2d(x64.permute(0, 3, 1, 2), w64.permute(0, 3, 1, 2), None, stride, pad)
    dy = rnd((n, geom.Ho, geom.Wo, cout), dtype, 4)
    y_lin.backward(dy.double().permute(0, 3, 1, 2))
    return x, w, geom, y_lin.detach(), dy, x64.grad, w64.grad


def _conv_fwd_check(x, w, geom, y_lin, dtype, what):
    cout = w.shape[0]
    scale, shift = torch.rand(cout) + 0.5, torch.randn(cout) * 0.1
    res = rnd((x.shape[0], geom.Ho, geom.Wo, cout), dtype, 3)
    y_ref = (y_lin * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1) + res.double().permute(0, 3, 1, 2)).clamp(min=0)
    y = ops.conv2d_fwd(x.to(DEV), w.to(DEV), geom, scale=scale.to(DEV), shift=shift.to(DEV), residual=res.to(DEV), relu=True)
    check(y, y_ref.permute(0, 2, 3, 1), dtype, 2, f"conv fwd {what}")


def _conv_dgrad_check(x, w, geom, dy, dx_ref, dtype, what, in_place):
    zero = torch.zeros((), dtype=torch.float64)
    w_t = w.permute(3, 1, 2, 0).contiguous()                        # [Cin, kh, kw, Cout]
    dres, mask = rnd(tuple(x.shape), dtype, 5), rnd(tuple(x.shape), dtype, 6)
    dx = ops.conv2d_dgrad(dy.to(DEV), w_t.to(DEV), geom, residual=dres.to(DEV), relu_mask=mask.to(DEV))
    check(dx, torch.where(mask.double() > 0, dx_ref + dres.double(), zero), dtype, 4, f"conv dgrad {what}")
    if in_place:
        # "dx = mask(dx + dgrad(dy))" in the caller's buffer (the backbone's stride-2 shortcut): the odd pixels, which no
        # tap reaches, must come back untouched
        pre = torch.where(mask.float() > 0, dres.float(), torch.zeros(())).to(dtype)
        buf = pre.clone().to(DEV)
        got = ops.conv2d_dgrad(dy.to(DEV), w_t.to(DEV), geom, residual=buf, relu_mask=mask.to(DEV), out=buf)
        assert got.data_ptr() == buf.data_ptr()
        check(buf, torch.where(mask.double() > 0, dx_ref + pre.double(), zero), dtype, 4, f"conv dgrad in place {what}")
        assert torch.equal(buf.cpu()[:, 1::2], pre[:, 1::2]), "pixels without taps were rewritten"


@pytest.mark.parametrize("c", **_params("nt128", call="conv_fwd"))
def test_nt128_wide_tile_conv(knobs, c):
    """Forward, input gradient (stride 1, stride 2 and in place) and weight gradient as test_conv2d_fwd_dgrad_wgrad, with
    the forward and the input gradient on the 128-wide tile (each has its own N: Cout, Cin)."""
    (d,) = V.cases("nt128", call="conv_dgrad", shape=c.shape, dtype=c.dtype)
    dtype = V.DTYPE[c.dtype]
    x, w, geom, y_lin, dy, dx_ref, dw_ref = _conv_inputs(c.shape, dtype)
    n, h, w_, cin, cout, k, stride, pad = c.shape
    _enter(knobs, c)
    _conv_fwd_check(x, w, geom, y_lin, dtype, c.shape)
    _enter(knobs, d)
    _conv_dgrad_check(x, w, geom, dy, dx_ref, dtype, c.shape, in_place=stride == 2 and k == 1)
    dw = torch.zeros((cout, k, k, cin), device=DEV)
    rs = torch.rand(cout) + 0.5
    ops.conv2d_wgrad_acc(dy.to(DEV), x.to(DEV), dw, geom, row_scale=rs.to(DEV))
    check(dw, dw_ref * rs.double().view(-1, 1, 1, 1), _out_dtype(dtype), math.sqrt(n * geom.Ho * geom.Wo), f"conv wgrad {c.shape}")


# ------------------------------------------------------------------------------------------------ NT, K split across blocks
@pytest.mark.parametrize("c", **_params("nt_splitk"))
def test_nt_short_launch_split_k(knobs, c):
    """FOD_NT_SPLITK = unset / 0 / 2 / 3 / 8: the split count the route reports is min(256 // tiles, cap, K // 256) (1 for
    0; K chunks that do not divide K among them), both epilogues of test_gemm_nt_short_launch, every call issued twice
    on one stream (the second finds the tickets the first left), and the tickets are zero afterwards."""
    r = _enter(knobs, c)
    M, N, K = c.shape
    tiles = -(-M // 64) * -(-N // 64)
    knob = c.knobs.get("FOD_NT_SPLITK")
    assert r.ksplit == (1 if knob == 0 else min(256 // tiles, 4 if knob is None else knob, K // 256))
    dtype = torch.bfloat16
    a, b = rnd((M, K), dtype, 7), rnd((N, K), dtype, 8)
    shift, res = torch.randn(N), rnd((M, N), dtype, 9)
    prod = a.double() @ b.double().t()
    ad, bd, sd, rd = a.to(DEV), b.to(DEV), shift.to(DEV), res.to(DEV)
    outs = [ops.gemm_nt(ad, bd, shift=sd, residual=rd) for _ in range(2)]
    outs32 = [ops.gemm_nt(ad, bd, relu=True, out_f32=True) for _ in range(2)]
    for i in range(2):
        check(outs[i], prod + shift.double() + res.double(), dtype, math.sqrt(K), f"nt split-K {c.shape} call {i}")
        check(outs32[i], prod.clamp(min=0), dtype, math.sqrt(K), f"nt split-K relu f32 {c.shape} call {i}")
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs32[0], outs32[1])
    tickets = ops._workspace(L.WS_NT_SPLIT_TICKETS, ad.device)
    assert int(tickets.abs().sum()) == 0, "split-K tickets were not left at zero"


# ------------------------------------------------------------------------------------------------ NT, 256-row kernel
@pytest.mark.parametrize("c", **_params("nt_big", call="gemm_nt"))
def test_nt_big_interleave_and_stages_dense(knobs, c):
    """Interleaved DMA requests crossed with the ring depth: (3 stages, off) and (2 stages, on) never run by default."""
    _enter(knobs, c)
    dtype = torch.bfloat16
    M, N, K = c.shape
    a, b = rnd((M, K), dtype, 1), rnd((N, K), dtype, 2)
    shift, res, mask = torch.randn(N), rnd((50, N), dtype, 3), rnd((M, N), dtype, 4)
    prod = a.double() @ b.double().t()
    acc = prod + shift.double() + res.double().repeat(M // 50 + 1, 1)[:M]
    ref = torch.where(mask.double() > 0, acc.clamp(min=0), torch.zeros((), dtype=torch.float64))
    out = ops.gemm_nt(a.to(DEV), b.to(DEV), shift=shift.to(DEV), residual=res.to(DEV), residual_row_mod=50, relu=True,
                      relu_mask=mask.to(DEV))
    check(out, ref, dtype, math.sqrt(K), f"nt big {c.shape}")
    out32 = ops.gemm_nt(a.to(DEV), b.to(DEV), shift=shift.to(DEV), out_f32=True)
    check(out32, prod + shift.double(), dtype, math.sqrt(K), f"nt big f32 out {c.shape}")


@pytest.mark.parametrize("c", **_params("nt_big", call="conv_fwd"))
def test_nt_big_interleave_and_stages_conv(knobs, c):
    (d,) = [d for d in V.cases("nt_big", call="conv_dgrad", shape=c.shape) if d.knobs == c.knobs]
    dtype = torch.bfloat16
    x, w, geom, y_lin, dy, dx_ref, _ = _conv_inputs(c.shape, dtype)
    _enter(knobs, c)
    _conv_fwd_check(x, w, geom, y_lin, dtype, c.shape)
    _enter(knobs, d)
    _conv_dgrad_check(x, w, geom, dy, dx_ref, dtype, c.shape, in_place=False)


# ------------------------------------------------------------------------------------------------ TN
def _thrice(run):
    outs = [tuple(t.clone() for t in run()) for _ in range(3)]
    torch.cuda.synchronize()
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b), float((a.float() - b.float()).abs().max())
    return outs[0]


def _tn_dense(c):
    """gemm_tn_acc with row scales and fused column sums, added to a gradient and written into zeroed outputs; in
    deterministic mode also bit-equal over three runs."""
    dtype = V.DTYPE[c.dtype]
    M, N1, K2 = c.shape
    g, x = rnd((M, N1), dtype, 1), rnd((M, K2), dtype, 2)
    rs = torch.rand(N1) + 0.5
    gd, xd, rsd = g.to(DEV), x.to(DEV), rs.to(DEV)
    prod = (g.double().t() @ x.double()) * rs.double()[:, None]
    colsum = g.double().sum(0)
    for zeroed in (False, True):
        dw0 = torch.zeros(N1, K2) if zeroed else torch.randn(N1, K2)
        cs0 = torch.zeros(N1) if zeroed else torch.randn(N1)

        def run():
            dw, cs = dw0.clone().to(DEV), cs0.clone().to(DEV)
            ops.gemm_tn_acc(gd, xd, dw, row_scale=rsd, colsum=cs, zeroed=zeroed)
            return dw, cs
        dw, cs = _thrice(run) if c.extra.get("det") else run()
        check(dw, dw0.double() + prod, _out_dtype(dtype), math.sqrt(M), f"tn {c.shape} zeroed={zeroed}")
        check(cs, cs0.double() + colsum, torch.float32, math.sqrt(M), f"tn colsum {c.shape} zeroed={zeroed}")


@pytest.mark.parametrize("c", **_params("tn128"))
def test_tn128_block_orders_and_split_counts(knobs, c):
    """The 128 x 128 kernel in XCD-grouped order with 23 and 15 M-splits (the grid is rounded up to a multiple of 8 splits
    and the tail blocks return early), with 8 in both orders, with forced rows per split; 23 splits also in
    deterministic mode, where partial tiles are counted and summed in order."""
    _enter(knobs, c)
    _tn_dense(c)


@pytest.mark.parametrize("c", **_params("tn_big", call="gemm_tn"))
def test_tn_big_with_the_workspace_dense(knobs, c):
    """The 8-wave kernel from 8192 rows on, where the wrappers hand the workspace over: partial-tile stores and the reduce
    launch on ragged N1 / K2 in both tile families, f32 atomics under FOD_TN_WS=0, deterministic mode."""
    _enter(knobs, c)
    _tn_dense(c)


@pytest.mark.parametrize("c", **_params("tn_big", call="conv_wgrad"))
def test_tn_big_with_the_workspace_conv(knobs, c):
    dtype = torch.bfloat16
    n, h, w_, cin, cout, k, stride, pad = c.shape
    x, w, geom, _, dy, _, dw_ref = _conv_inputs(c.shape, dtype)
    rs = torch.rand(cout) + 0.5
    _enter(knobs, c)
    for zeroed in (False, True):
        dw0 = torch.zeros(cout, k, k, cin) if zeroed else torch.randn(cout, k, k, cin)
        dw = dw0.clone().to(DEV)
        ops.conv2d_wgrad_acc(dy.to(DEV), x.to(DEV), dw, geom, row_scale=rs.to(DEV), zeroed=zeroed)
        check(dw, dw0.double() + dw_ref * rs.double().view(-1, 1, 1, 1), dtype, math.sqrt(n * geom.Ho * geom.Wo),
              f"tn big conv wgrad {c.shape} zeroed={zeroed}")


# ------------------------------------------------------------------------------------------------ layer norm
@pytest.mark.parametrize("rows", V.LN_ROWS)
@pytest.mark.parametrize("D", V.LN_WIDTHS)
@pytest.mark.parametrize("dtype", V.BOTH)
def test_layernorm_every_width_and_the_many_row_kernels(knobs, dtype, D, rows):
    """Forward (residual per row and broadcast with res_row_div) and backward at every instantiated width, below and from
    the many-row threshold on (8192 rows: 16 or 8 lanes per row, a wave walks FOD_LN_BWD_GROUPS row groups), against
    float64 autograd of F.layer_norm on the stored sum.  mean / rstd are computed by torch from the stored sum, as the
    fused linear-norm tests do, and the kernel's own statistics are held against them."""
    mine = V.cases("layernorm", shape=(rows, D), dtype=dtype)
    assert len(mine) == (3 if rows >= 8192 else 1)
    dtype = V.DTYPE[dtype]
    x, r = rnd((rows, D), dtype, 1), rnd((rows, D), dtype, 2)
    gamma, beta = torch.rand(D) + 0.5, torch.randn(D) * 0.1
    s_ref = (x.float() + r.float()).to(dtype)
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    y, s, mean_k, rstd_k = ops.layernorm_fwd(xd, gd, bd, residual=r.to(DEV))
    check(s, s_ref, dtype, 1, "ln sum")
    s64 = s.detach().cpu().double().requires_grad_(True)            # the stored sum is what was normalised
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y_ref = F.layer_norm(s64, (D,), g64, b64, 1e-5)
    check(y, y_ref, dtype, 2, "ln fwd")
    mean = s.float().mean(-1).contiguous()
    rstd = (s.float().var(-1, unbiased=False) + 1e-5).rsqrt().contiguous()
    assert torch.allclose(mean_k, mean, atol=1e-4) and torch.allclose(rstd_k, rstd, rtol=1e-4)
    rb = rnd(((rows + 4) // 5, D), dtype, 4)                        # row m adds residual row m // 5
    yb, sb, _, _ = ops.layernorm_fwd(xd, gd, bd, residual=rb.to(DEV), res_row_div=5)
    sb_ref = (x.float() + rb.float().repeat_interleave(5, 0)[:rows]).to(dtype)
    check(sb, sb_ref, dtype, 1, "ln bcast sum")
    check(yb, F.layer_norm(sb.cpu().double(), (D,), gamma.double(), beta.double(), 1e-5), dtype, 2, "ln bcast")
    dy = rnd((rows, D), dtype, 3)
    y_ref.backward(dy.double())
    for c in mine:
        knobs(**c.knobs)
        for name, value in c.knobs.items():
            assert L.knob(name) == str(value)
        dg, db = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
        dx = ops.layernorm_bwd(dy.to(DEV), s, mean, rstd, gd, dg, db)
        check(dx, s64.grad, dtype, 4, f"ln dx {c.knobs}")
        check(dg, g64.grad, torch.float32, math.sqrt(rows), f"ln dgamma {c.knobs}")
        check(db, b64.grad, torch.float32, math.sqrt(rows), f"ln dbeta {c.knobs}")


# ------------------------------------------------------------------------------------------------ attention
@functools.lru_cache(maxsize=None)
def _attn_problem(shape, dtype, drop):
    """Inputs and the float64 reference (output and gradients) of one attention problem, shared by the knob sets that
    run it; nobody writes to what this returns."""
    B, H, Tq, S, parts = shape
    E = H * 32
    q1, k1, v = rnd((B, Tq, E), dtype, 1), rnd((B, S, E), dtype, 2), rnd((B, S, E), dtype, 3)
    q2 = rnd((B, Tq, E), dtype, 4) if parts == 2 else None
    k2 = rnd((B, S, E), dtype, 5) if parts == 2 else None
    scale = 1.0 / math.sqrt(32 * parts)
    leaves = [t.double().requires_grad_(True) if t is not None else None for t in (q1, k1, v, q2, k2)]
    if drop:
        seed = 0x1234567890ABCDEF
        keep = _drop_keep_mask(B, H, Tq, S, seed, drop).double()
        heads = lambda t: t.view(t.shape[0], t.shape[1], H, 32).transpose(1, 2)
        sc = heads(leaves[0]) @ heads(leaves[1]).transpose(-1, -2)
        if parts == 2:
            sc = sc + heads(leaves[3]) @ heads(leaves[4]).transpose(-1, -2)
        prob = torch.softmax(sc * scale, dim=-1) * keep / (1 - drop)
        o_ref = (prob @ heads(leaves[2])).transpose(1, 2).reshape(B, Tq, E)
    else:
        seed = 0
        o_ref = _attn_ref(leaves[0], leaves[1], leaves[2], scale, leaves[3], leaves[4])
    dout = rnd((B, Tq, E), dtype, 6)
    o_ref.backward(dout.double())
    grads = [None if t is None else t.grad for t in leaves]
    return (q1, k1, v, q2, k2), dout, scale, seed, o_ref.detach(), grads


def _attn_run_and_check(c, calls=1):
    """Forward, then the backward consuming the forward's own output; bounds of test_attention_fwd_bwd."""
    dtype = V.DTYPE[c.dtype]
    B, H, Tq, S, parts = c.shape
    drop = c.extra.get("drop", 0.0)
    (q1, k1, v, q2, k2), dout, scale, seed, o_ref, grads = _attn_problem(c.shape, dtype, drop)
    g = lambda t: None if t is None else t.to(DEV)
    dq1, dk1, dv, dq2, dk2, do = g(q1), g(k1), g(v), g(q2), g(k2), g(dout)
    kw = dict(drop_p=drop, drop_seed=seed) if drop else {}
    fwd = [ops.attn_fwd(dq1, dk1, dv, scale, dq2, dk2, **kw) for _ in range(calls)]
    bwd = [ops.attn_bwd(dq1, dk1, dv, o, do, lse2, scale, dq2, dk2, **kw) for o, lse2 in fwd]
    sc = math.sqrt(max(Tq, S)) * 0.5
    for i in range(calls):
        check(fwd[i][0], o_ref, dtype, 1, f"attn fwd {c.shape} call {i}")
        for name, got, want in zip(("dq1", "dk1", "dq2", "dk2", "dv"), bwd[i], (grads[0], grads[1], grads[3], grads[4], grads[2])):
            if want is not None:
                check(got, want, dtype, sc, f"{name} {c.shape} call {i}")
    return fwd, bwd


@pytest.mark.parametrize("c", **_params("attn_family"))
def test_attention_kernel_families(knobs, c):
    """bf16 attention on the kernels the defaults never pick at these shapes: the four-wave LDS forward, the plain
    forward / dq kernels without dropout, the plain dK/dV kernel (with and without dropout, split and not), the
    prefetching dK/dV kernel behind the plain forward."""
    _enter(knobs, c)
    _attn_run_and_check(c)


@pytest.mark.parametrize("c", **_params("attn_extreme"))
def test_attention_lds_forwards_rare_branches(knobs, c):
    """test_attention_forward_deferred_max_and_extreme_scores at 600 queries, where the LDS forwards run (at its own 300
    queries the keys are split over a block's waves instead): forced rescales, hugely negative and positive rows, the
    log-sum-exp -- on the four-wave and the eight-wave forward."""
    _enter(knobs, c)
    deferred_max_and_extreme_scores(c.shape[4], c.shape[:4])


@pytest.mark.parametrize("c", **_params("attn_saturated"))
def test_attention_four_wave_forward_saturated_softmax(knobs, c):
    _enter(knobs, c)
    saturated_softmax_forward_backward(c.shape)


def _attn_tickets_are_zero(what):
    tickets = ops._attn_split_workspace(torch.device(DEV), 1)[1]
    assert int(tickets.abs().sum()) == 0, f"{what}: key-split tickets were not left at zero"


@pytest.mark.parametrize("c", **_params("attn_ksplit"))
def test_attention_keys_split_across_blocks(knobs, c):
    """2, 3, 4 and 8 splits, a last chunk of 208 and of 44 keys, exactly two tiles, Tq at 512, and one key short of a
    split; every call twice on one stream (the second finds the tickets and the scratch the first left)."""
    r = _enter(knobs, c)
    assert (r.ksplit - 1) * r.kchunk < c.shape[3] <= r.ksplit * r.kchunk
    fwd, bwd = _attn_run_and_check(c, calls=2)
    assert torch.equal(fwd[0][0], fwd[1][0]) and torch.equal(fwd[0][1], fwd[1][1])
    for a, b in zip(bwd[0], bwd[1]):
        assert a is None or torch.equal(a, b)
    _attn_tickets_are_zero(V.case_id(c))


@pytest.mark.parametrize("c", **_params("attn_strided"))
def test_attention_strided_operands(knobs, c):
    """What the wrappers promise beyond contiguous operands: q1 / k1 / v / q2 as column slices of one [B, T, 4E] buffer,
    k2 a batch-shared [S, E] table, dk1 / dv written into slots of a larger buffer, dk2 per batch element into a slot of
    its own.  Same kernel, same arithmetic: every result equals the contiguous call's bit for bit, and no byte outside
    the slots changes."""
    _enter(knobs, c)
    dtype = torch.bfloat16
    B, H, T, S, parts = c.shape
    assert T == S and parts == 2
    E = H * 32
    packed = rnd((B, T, 4 * E), dtype, 1).to(DEV)
    q1, k1, v, q2 = (packed[:, :, i * E:(i + 1) * E] for i in range(4))
    k2 = rnd((S, E), dtype, 5).to(DEV)
    dout = rnd((B, T, E), dtype, 6).to(DEV)
    scale = 1.0 / math.sqrt(64)
    assert not q1.is_contiguous() and q1.stride() == (T * 4 * E, 4 * E, 1)
    # the contiguous call (k2 repeated per batch element)
    cq1, ck1, cv, cq2 = (t.contiguous() for t in (q1, k1, v, q2))
    ck2 = k2.unsqueeze(0).expand(B, S, E).contiguous()
    o_c, lse_c = ops.attn_fwd(cq1, ck1, cv, scale, cq2, ck2)
    ref = ops.attn_bwd(cq1, ck1, cv, o_c, dout, lse_c, scale, cq2, ck2)
    # against float64, so that "equal" is not two equal mistakes
    o64 = _attn_ref(cq1.cpu().double(), ck1.cpu().double(), cv.cpu().double(), scale, cq2.cpu().double(), ck2.cpu().double())
    check(o_c, o64, dtype, 1, f"attn fwd {c.shape}")
    # the strided call
    sentinel = 0x7F7F                                               # bf16 3.4e38 in every element
    slots = torch.full((B, S, 4 * E), sentinel, dtype=torch.int16, device=DEV).view(dtype)
    slots2 = torch.full((B, S, 2 * E), sentinel, dtype=torch.int16, device=DEV).view(dtype)
    dk1_out, dv_out, dk2_out = slots[:, :, E:2 * E], slots[:, :, 2 * E:3 * E], slots2[:, :, E:]
    o_s, lse_s = ops.attn_fwd(q1, k1, v, scale, q2, k2)
    got = ops.attn_bwd(q1, k1, v, o_s, dout, lse_s, scale, q2, k2, dk1_out=dk1_out, dv_out=dv_out, dk2_out=dk2_out)
    assert torch.equal(o_s, o_c) and torch.equal(lse_s, lse_c)
    assert got[1].data_ptr() == dk1_out.data_ptr() and got[4].data_ptr() == dv_out.data_ptr() and got[3].data_ptr() == dk2_out.data_ptr()
    for name, a, b in zip(("dq1", "dk1", "dq2", "dk2", "dv"), got, ref):
        assert torch.equal(a, b), (name, float((a.float() - b.float()).abs().max()))
    raw, raw2 = slots.view(torch.int16), slots2.view(torch.int16)
    assert bool((raw[:, :, :E] == sentinel).all()) and bool((raw[:, :, 3 * E:] == sentinel).all()), "bytes outside the dk1 / dv slots changed"
    assert bool((raw2[:, :, :E] == sentinel).all()), "bytes outside the dk2 slot changed"
    if c.expect["ksplit"] > 1:
        _attn_tickets_are_zero(V.case_id(c))


# ------------------------------------------------------------------------------------------------ fp8 attention
@pytest.mark.parametrize("c", **_params("fp8_stage2"))
def test_attention_fp8_two_tiles_per_barrier(knobs, c):
    """FOD_FP8_STAGE=2 (odd and even tile counts, a single key, a last stage with one tile): everything
    test_attention_fp8_forward_and_backward asserts.  The knob has no route query; it is read back."""
    _enter(knobs, c)
    assert L.knob("FOD_FP8_STAGE") == "2"
    attention_fp8_forward_and_backward(c.shape, c.extra["peaked"])
