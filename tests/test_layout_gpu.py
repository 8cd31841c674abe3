"""The kernels that move and reshape data (csrc/elementwise.hip) and the optimizer's (csrc/optim.hip), branch by branch,
against a plain CPU computation of the same operation.

The cases live in tests/layout_cases.py; tests/test_permute_plan_cpu.py holds each case against a Python statement of the
kernel's path conditions and counts the cases per path, so that "this case reaches the rows path" is checked, not
hoped.  Copies, casts, element-wise ops, layout changes and pooling are one f32 operation (or none) and one
round-to-nearest-even cast: the reference does the same f32 operations in the same order on the CPU and the results are
compared with torch.equal.  Destinations are pre-filled with a sentinel and every element outside a job's region must
still hold it.  Sums (column sums, gradient norms) are compared with float64 under bounds derived where they are used."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import layout_cases as LC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

if torch.cuda.is_available():
    from future_od.native import functional as Fn
    from future_od.native import lib as L
    from future_od.native import ops
    from test_kernels_gpu import check


@pytest.fixture(autouse=True)
def _mode_is_restored():
    prev = ops.is_deterministic()
    yield
    ops.set_deterministic(prev)


def _same(got, want, what):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not torch.equal(got, want):
        bad = (got != want).flatten().nonzero().flatten()
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.numel()}/{got.numel()} elements differ, first at flat index {i}: "
                             f"got {float(got.flatten()[i])!r}, want {float(want.flatten()[i])!r}")


def _guarded(t, off=0, tail=8):
    """A device copy of `t` as a contiguous view starting `off` elements into a buffer full of sentinels: (buffer, view)."""
    buf = torch.full((off + t.numel() + tail,), LC.SENTINEL, dtype=t.dtype, device=DEV)
    view = buf[off:off + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def _guards_intact(buf, off, n, what):
    raw = buf.cpu()
    assert bool((raw[:off] == LC.SENTINEL).all()) and bool((raw[off + n:] == LC.SENTINEL).all()), f"{what}: wrote outside its output"


# ------------------------------------------------------------------------------------------------ fod_multi_permute3
@functools.lru_cache(maxsize=None)
def _permute_problem(name):
    """(source buffer, scale, expected region) of a case, on the CPU; nobody writes to what this returns."""
    c = LC.permute(name)
    g = torch.Generator().manual_seed(LC.seed_of(name))
    src = torch.randn(c.src_off + LC.src_span(c) + 3, generator=g).to(LC.DTYPE[c.src])
    scale = torch.rand(c.dims[c.axis], generator=g) + 0.5 if c.axis >= 0 else None
    ref = torch.as_strided(src, c.dims, c.sstr, c.src_off).clone().float()
    if scale is not None:
        shape = [1, 1, 1]
        shape[c.axis] = -1
        ref = ref * scale.view(shape)                               # one f32 multiply
    ref[:, c.valid1:, :] = 0
    ref[:, :, c.valid2:] = 0
    return src, scale, ref.to(LC.DTYPE[c.dst])                      # one round-to-nearest-even cast


def _launch_permute(names):
    """The cases as ONE job table built by the production host code, one launch; every destination buffer is compared
    whole: the job's region with the reference, everything else with the sentinel it held."""
    cases = [LC.permute(n) for n in names]
    bufs, jobs = {}, []
    for c in cases:
        src, scale, ref = _permute_problem(c.name)
        key = c.share or c.name
        if key not in bufs:
            n = LC.dst_numel(c)
            bufs[key] = (torch.full((n,), LC.SENTINEL, dtype=LC.DTYPE[c.dst]),
                         torch.full((n,), LC.SENTINEL, dtype=LC.DTYPE[c.dst], device=DEV))
        want, got = bufs[key]
        assert c.dst_off + LC.dst_span(c) <= want.numel() and c.src_off + LC.src_span(c) <= src.numel()
        torch.as_strided(want, c.dims, c.dstr + (1,), c.dst_off).copy_(ref)
        jobs.append(Fn._Job(src.to(DEV)[c.src_off:], got[c.dst_off:], c.dims, c.sstr, dstr=c.dstr, valid1=c.valid1,
                            valid2=c.valid2, scale=None if scale is None else scale.to(DEV), axis=c.axis))
    tab = Fn._Prepared()._build_tables(jobs)
    assert tab[3] == sum(LC.permute_tiles(c.dims, c.sstr) for c in cases)
    L.call("fod_multi_permute3", ops.ptr(tab[0]), ops.ptr(tab[1]), ops.ptr(tab[2]), tab[3], ops.stream())
    torch.cuda.synchronize()
    for c in cases:
        want, got = bufs[c.share or c.name]
        region = torch.as_strided(got.cpu(), c.dims, c.dstr + (1,), c.dst_off)
        _same(region, _permute_problem(c.name)[2], f"{c.name} ({c.path}, {c.epi})")
    for key, (want, got) in bufs.items():
        _same(got, want, f"buffer {key}: an element outside the jobs' regions changed")
    return jobs


@pytest.mark.parametrize("name", [c.name for c in LC.PERMUTE])
def test_multi_permute_every_path(name):
    """One job per launch: both transposing paths with both store epilogues, the rows path, the generic path, the four
    dtype pairs, valid1 / valid2 padding, the three scale axes, custom destination strides and offset views.  Where the
    job is expressible as one fod_permute3_cast call the two kernels must agree bit for bit as well."""
    c = LC.permute(name)
    (job,) = _launch_permute([name])
    if LC.is_single_call(c):
        out = ops.permute3_cast(job.src, LC.DTYPE[c.dst], c.dims, c.sstr, valid2=c.valid2, scale=job.scale, scale_axis=c.axis)
        _same(out, _permute_problem(name)[2], f"{name}: permute3_cast")


def test_multi_permute_mixed_table():
    """Jobs of every kind in a single launch, among them two pairs that write different slots of one buffer."""
    kinds = {LC.permute(n).path for n in LC.MIXED_TABLE}
    assert kinds == {"t16", "t32", "rows", "generic"} and len(LC.MIXED_TABLE) >= 12
    _launch_permute(LC.MIXED_TABLE)


# ------------------------------------------------------------------------------------------------ fod_permute3_cast
@pytest.mark.parametrize("pair", LC.PAIRS, ids=["-".join(p) for p in LC.PAIRS])
def test_permute3_cast_dtype_pairs_scale_axes_padding(pair):
    src_t, dst_t = LC.DTYPE[pair[0]], LC.DTYPE[pair[1]]
    for dims, sstr, valid2 in LC.P3_SHAPES:
        v2 = dims[2] if valid2 is None else valid2
        g = torch.Generator().manual_seed(sum(dims))
        src = torch.randn(1 + sum((d - 1) * s for d, s in zip(dims, sstr)), generator=g).to(src_t)
        for axis in LC.P3_AXES:
            scale = torch.rand(dims[axis], generator=g) + 0.5 if axis >= 0 else None
            ref = torch.as_strided(src, dims, sstr).clone().float()
            if scale is not None:
                shape = [1, 1, 1]
                shape[axis] = -1
                ref = ref * scale.view(shape)
            ref[:, :, v2:] = 0
            buf, out = _guarded(torch.zeros(dims, dtype=dst_t), off=8)
            got = ops.permute3_cast(src.to(DEV), dst_t, dims, sstr, valid2=valid2, scale=None if scale is None else scale.to(DEV),
                                    scale_axis=axis, out=out)
            _same(got, ref.to(dst_t), f"permute3_cast {pair} {dims} {sstr} valid2={valid2} axis={axis}")
            _guards_intact(buf, 8, out.numel(), f"permute3_cast {dims}")


# ------------------------------------------------------------------------------------------------ fod_eltwise
def _ew_rows(rows, div, mod):
    m = torch.arange(rows)
    if div:
        m = m // div                                                # res_row divides first, then takes the modulus
    if mod:
        m = m % mod
    return m


def _ew_ref(op, a, b, c, alpha):
    """The kernel's f32 operations in its order, then the cast.  b is already gathered per row."""
    av = a.float()
    bv = None if b is None else b.float()
    if op == "ADD":
        r = av + bv
    elif op == "MUL":
        r = av * bv
    elif op == "RELU_MASK":
        r = torch.where(bv > 0, av, torch.zeros(()))
    elif op == "SCALE":
        r = torch.tensor(alpha, dtype=torch.float32) * av
    elif op == "ADD3":
        r = (av + bv) + c.float()
    elif op == "COPY_B":
        r = bv.clone()
    else:
        r = av.clamp(min=0)
    return r.to(a.dtype)


@pytest.mark.parametrize("shape", LC.EW_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", LC.BOTH)
def test_eltwise_every_op_both_kernels(dtype, shape):
    """All seven ops on the 16-byte kernel and on the scalar one (a row length that is no multiple of the vector width, or
    one operand starting one element into its buffer), b per row / b_row_mod / b_row_div / both, out aliasing a."""
    rows, cols = shape
    dt = LC.DTYPE[dtype]
    g = torch.Generator().manual_seed(rows * 1000 + cols)
    a, b, c = (torch.randn(rows, cols, generator=g).to(dt) for _ in range(3))
    seen = set()
    for op in LC.EW_OPS:
        has_b = op in LC.EW_NEEDS_B
        for operand in LC.EW_OPERANDS:
            if operand == "b+1" and not has_b:
                continue
            for bname, (div, mod) in LC.EW_BCAST.items() if has_b else [("none", (0, 0))]:
                for alpha in LC.EW_ALPHAS if op == "SCALE" else (1.0,):
                    what = f"{op} {dtype} {shape} {operand} b:{bname} alpha={alpha}"
                    seen.add(LC.eltwise_kernel(dtype, shape, operand, has_b))
                    _, a_d = _guarded(a, off=1 if operand == "a+1" else 0)
                    b_d = b_rows = None
                    if has_b:
                        b_rows = b[:LC.eltwise_b_rows(rows, div, mod)]
                        _, b_d = _guarded(b_rows, off=1 if operand == "b+1" else 0)
                    c_d = c.to(DEV) if op == "ADD3" else None
                    off = 1 if operand == "out+1" else 0
                    obuf, out = _guarded(torch.zeros(rows, cols, dtype=dt), off=off)
                    assert (a_d.data_ptr() % 16 != 0) == (operand == "a+1") and (out.data_ptr() % 16 != 0) == (operand == "out+1")
                    got = ops.eltwise(LC.EW_OPS.index(op), a_d, b_d, c_d, b_row_div=div, b_row_mod=mod, alpha=alpha, out=out)
                    ref = _ew_ref(op, a, b_rows[_ew_rows(rows, div, mod)] if has_b else None, c, alpha)
                    _same(got, ref, what)
                    _guards_intact(obuf, off, out.numel(), what)
    assert seen == {LC.eltwise_kernel(dtype, shape, "aligned", True), "scalar"}
    for op in ("COPY_B", "ADD"):                                    # in place: out is a (every thread reads what it writes)
        for bname, (div, mod) in LC.EW_BCAST.items():
            b_rows = b[:LC.eltwise_b_rows(rows, div, mod)]
            abuf, a_d = _guarded(a)
            got = ops.eltwise(LC.EW_OPS.index(op), a_d, b_rows.to(DEV), b_row_div=div, b_row_mod=mod, out=a_d)
            assert got.data_ptr() == a_d.data_ptr()
            _same(got, _ew_ref(op, a, b_rows[_ew_rows(rows, div, mod)], None, 1.0), f"{op} in place {dtype} {shape} b:{bname}")
            _guards_intact(abuf, 0, a_d.numel(), f"{op} in place")


# ------------------------------------------------------------------------------------------------ layout
def _nhwc_ref(frames, cp, dtype):
    """f32 [F, C, H, W] -> dtype [F, H, W, cp], zero channels behind C."""
    f, c, h, w = frames.shape
    out = torch.zeros(f, h, w, cp)
    out[..., :c] = frames.permute(0, 2, 3, 1)
    return out.to(dtype)


def _normalised(u8, c):
    """((x / 255) - mean) / std in f32 -- through numpy, whose f32 division by a scalar is a division (torch's CPU kernel
    may multiply by the reciprocal, which is not the operation the kernel promises to reproduce)."""
    x = u8.numpy().astype(np.float32) / np.float32(255)
    mean = np.asarray(LC.MEAN[:c], dtype=np.float32).reshape(1, c, 1, 1)
    std = np.asarray(LC.STD[:c], dtype=np.float32).reshape(1, c, 1, 1)
    return torch.from_numpy((x - mean) / std)


@pytest.mark.parametrize("case", LC.NCHW, ids=lambda c: f"{'x'.join(map(str, c[0]))}-cp{c[1]}-{c[2]}-{c[3]}")
def test_nchw_to_nhwc_both_kernels(case):
    """The four-pixels-per-thread bf16 kernel and the general one for each reason the fast one is not taken."""
    (f, c, h, w), cp, dtype, _ = case
    v = torch.randn(f, c, h, w, generator=torch.Generator().manual_seed(f * h * w + cp))
    _same(ops.nchw_to_nhwc(v.to(DEV), LC.DTYPE[dtype], cp), _nhwc_ref(v, cp, LC.DTYPE[dtype]), f"nchw_to_nhwc {case}")


@pytest.mark.parametrize("source", ["f32", "u8"])
@pytest.mark.parametrize("clip", LC.CLIPS, ids=lambda c: f"B{c[0]}-L{c[1]}-cut{c[2]}-{c[3]}x{c[4]}x{c[5]}")
def test_clip_to_nhwc_frame_major(clip, source):
    """[B, L, C, H, W] -> [(l, b), H, W, Cp]: the frame-major mapping of both f32 kernels and of the uint8 one, from a whole
    clip and from a [:, 1:4] slice of a longer one.  uint8 frames are normalised on the fly, bit-identical to
    ((x / 255) - mean) / std in f32; bf16 outputs equal that value cast to bf16."""
    B, L, cut, C, H, W = clip
    g = torch.Generator().manual_seed(B * 100 + L * 10 + H)
    if source == "u8":
        whole = torch.randint(0, 256, (B, L, C, H, W), generator=g, dtype=torch.uint8)
        whole[0, -1, 0].view(-1)[:2] = torch.tensor([0, 255], dtype=torch.uint8)
    else:
        whole = torch.randn(B, L, C, H, W, generator=g)
    take = (lambda t: t[:, cut[0]:cut[1]]) if cut else (lambda t: t)
    video, video_d = take(whole), take(whole.to(DEV))
    assert video_d.is_contiguous() == (cut is None)
    l = video.shape[1]
    frames = video.permute(1, 0, 2, 3, 4).reshape(l * B, C, H, W)                   # ordered (l, b)
    frames = _normalised(frames, C) if source == "u8" else frames
    kw = dict(mean=torch.tensor(LC.MEAN[:C], device=DEV), std=torch.tensor(LC.STD[:C], device=DEV)) if source == "u8" else {}
    for dtype, cp in LC.CLIP_OUT:
        if cp < C:
            continue
        got = ops.clip_to_nhwc_frame_major(video_d, LC.DTYPE[dtype], cp, **kw)
        _same(got, _nhwc_ref(frames, cp, LC.DTYPE[dtype]), f"frame major {clip} {source} -> {dtype} cp={cp}")


@pytest.mark.parametrize("case", LC.POOL, ids=lambda c: f"{c[0]}-C{c[1]}-{c[2]}")
def test_maxpool_both_kernels_small_frames(case):
    """The 16-byte kernel and the scalar one at 1, 2, 7 and 8 rows and columns, on inputs that are all negative (a window
    padded with 0 instead of -inf would show).  Pooling selects a value: exact."""
    dtype, C, _ = case
    g = torch.Generator().manual_seed(C)
    for H in LC.POOL_HW:
        for W in LC.POOL_HW:
            x = (-(torch.randn(2, H, W, C, generator=g).abs() + 0.25)).to(LC.DTYPE[dtype])
            ref = F.max_pool2d(x.float().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous().to(LC.DTYPE[dtype])
            assert float(ref.max()) < 0
            _same(ops.maxpool3x3s2(x.to(DEV)), ref, f"maxpool {case} {H}x{W}")


# ------------------------------------------------------------------------------------------------ fod_colsum_groups_multi
@pytest.mark.parametrize("case", LC.COLSUM, ids=lambda c: "jobs{}-groups{}-rows{}-N{}".format(*c))
def test_colsum_groups_multi(case):
    """out_j[g] = sum of the rows of group g of G_j, bf16 in and out, against the float64 sum of the same bf16 inputs.
    Bound: |err| <= 2^-8 |ref| + 2^-17 sum|x| -- one bf16 rounding of the result, and f32 accumulation of at most 128 terms
    (n * 2^-24 * sum|x|).  Every job has inputs of its own and one job is all zero: a row of another group or another job
    that leaked into a sum would break the bound (the zero job must come out exactly zero)."""
    jobs, groups, gr, N = case
    gs, outs = [], []
    for j in range(jobs):
        x = torch.randn(groups * gr, N, generator=torch.Generator().manual_seed(100 * j + gr + N)).to(torch.bfloat16)
        if j == 1:
            x.zero_()
        gs.append(x)
        outs.append(_guarded(torch.zeros(groups, N, dtype=torch.bfloat16), off=8))
    ops.colsum_groups_multi([(x.to(DEV), o[1]) for x, o in zip(gs, outs)], groups, gr, N)
    for j, (x, (buf, out)) in enumerate(zip(gs, outs)):
        x64 = x.double().view(groups, gr, N)
        ref, mass = x64.sum(1), x64.abs().sum(1)
        err = (out.cpu().double() - ref).abs()
        bound = 2.0 ** -8 * ref.abs() + 2.0 ** -17 * mass
        assert bool((err <= bound).all()), (case, j, float((err - bound).max()), float(err.max()))
        _guards_intact(buf, 8, out.numel(), f"colsum {case} job {j}")


# ------------------------------------------------------------------------------------------------ reference points, box head
def _close(a, b, atol, rtol, what):
    np.testing.assert_allclose(a.detach().double().cpu().numpy(), b.detach().double().cpu().numpy(), atol=atol, rtol=rtol,
                               err_msg=what)


@pytest.mark.parametrize("ref_rows", LC.HEAD_REF_ROWS)
@pytest.mark.parametrize("D", LC.HEAD_D)
@pytest.mark.parametrize("dtype", LC.BOTH)
def test_refpoint_sine_and_box_finish_shared_points_and_saturation(dtype, D, ref_rows):
    """test_heads_gpu.py::test_refpoint_sine_and_box_finish in both dtypes, at both widths, from one row to more rows than
    a block has threads, with reference points shared by three rows each (r % ref_rows, and the dref sum over the rows
    that share a point), with and without dref_extra, and with logits of +-20 (f32 sigmoid exactly 1, or below the
    clamp): the clamp branches of inv_sigmoid (through boxes) and of inv_sigmoid_grad (through dref, compared directly)
    against autograd through the oracle's inverse_sigmoid(eps=1e-5), in float64, from the same (rounded) inputs.  f32: the bounds of the test named above; bf16:
    tol(bfloat16) on what is stored in bf16, the f32 bounds on the f32 outputs that do not depend on a bf16 rounding."""
    from oracle import stdetr as O
    from oracle import thirdparty as tp
    dt = LC.DTYPE[dtype]
    Lv = 3
    g = torch.Generator().manual_seed(ref_rows * 7 + D)
    logit = torch.randn(ref_rows, 2, generator=g)
    for i, sat in enumerate(LC.HEAD_SATURATED[:ref_rows]):
        logit[i] = torch.tensor(sat)
    logit = logit.to(dt)
    dsine = torch.randn(ref_rows, D, generator=g).to(dt)
    ref_d, sine_d = ops.refpoint_sine_fwd(logit.to(DEV), D)
    l64 = logit.double().requires_grad_(True)
    ref = l64.sigmoid()
    sine = O.query_sine_embed(ref[:, None, :], D)[:, 0]
    _close(ref_d, ref, 1e-5, 1e-5, "ref")
    if dtype == "f32":
        _close(sine_d, sine, 2e-5, 1e-5, "sine")
    else:
        check(sine_d, sine, dt, 1, "sine")
    (g_sine,) = torch.autograd.grad((sine * dsine.double()).sum(), l64, retain_graph=True)
    assert bool(torch.isfinite(g_sine).all())
    dlogit = ops.refpoint_sine_bwd(dsine.to(DEV), ref_d, None)
    if dtype == "f32":
        _close(dlogit, g_sine, 2e-4, 1e-4, "dlogit without dref_extra")
    else:
        check(dlogit, g_sine, dt, 1, "dlogit without dref_extra")
    for shared in LC.HEAD_SHARED:
        R = shared * ref_rows
        t = torch.randn(Lv, R, 4, generator=g).to(dt)
        dboxes = torch.randn(Lv, R, 4, generator=g)
        t64 = t.double().requires_grad_(True)
        rl = tp.inverse_sigmoid(ref).repeat(shared, 1)                          # row r uses point r % ref_rows
        boxes = torch.cat([t64[..., :2] + rl, t64[..., 2:]], -1).sigmoid()
        dt_ref, g_all = torch.autograd.grad((sine * dsine.double()).sum() + (boxes * dboxes.double()).sum(), [t64, l64],
                                            retain_graph=True)
        assert bool(torch.isfinite(dt_ref).all()) and bool(torch.isfinite(g_all).all())
        what = f"{dtype} D={D} ref_rows={ref_rows} shared={shared}"
        boxes_d = ops.box_finish_fwd(t.to(DEV), ref_d, Lv)
        _close(boxes_d, boxes, 1e-6, 1e-5, "boxes " + what)
        dt_d, dref_d = ops.box_finish_bwd(dboxes.to(DEV), boxes_d, ref_d, dt)
        assert dt_d.dtype == dt and dref_d.shape == (ref_rows, 2)
        # dref itself, with the kernel's own f32 reference points as the leaf (refpoint_sine_bwd multiplies it by
        # sg * (1 - sg), which is 0 at a saturated point: only here do the clamp branches of inv_sigmoid_grad show).
        # dref = (sum of at most 9 terms g) * d inverse_sigmoid / d ref; each g within the dt bound (atol 1e-6, rtol 1e-4)
        leaf = ref_d.cpu().double().requires_grad_(True)
        rl_leaf = tp.inverse_sigmoid(leaf)
        b_leaf = torch.cat([t.double()[..., :2] + rl_leaf.repeat(shared, 1), t.double()[..., 2:]], -1).sigmoid()
        (dref_ref,) = torch.autograd.grad((b_leaf * dboxes.double()).sum(), leaf, retain_graph=True)
        (slope,) = torch.autograd.grad(rl_leaf.sum(), leaf)
        assert bool(torch.isfinite(dref_ref).all()) and bool(((slope[:len(LC.HEAD_SATURATED[:ref_rows])] - 1).abs() < 1e-6).all())   # clamped: 1/x or 1/(1-x) alone
        g_abs = (dboxes.double() * b_leaf.detach() * (1 - b_leaf.detach()))[..., :2].abs().view(Lv, shared, ref_rows, 2).sum((0, 1))
        bound = slope * (Lv * shared * 1e-6 + 1e-4 * g_abs) + 1e-7
        err = (dref_d.cpu().double() - dref_ref).abs()
        assert bool((err <= bound).all()), ("dref " + what, float((err - bound).max()), float(err.max()))
        dlogit = ops.refpoint_sine_bwd(dsine.to(DEV), ref_d, dref_d)
        if dtype == "f32":
            _close(dt_d, dt_ref, 1e-6, 1e-4, "dt " + what)
            _close(dlogit, g_all, 2e-4, 1e-4, "dlogit " + what)
        else:
            check(dt_d, dt_ref, dt, 1, "dt " + what)
            check(dlogit, g_all, dt, 1, "dlogit " + what)


# ------------------------------------------------------------------------------------------------ optimizer
def _offset_view(values, off):
    buf = torch.full((off + values.numel() + 4,), LC.SENTINEL, device=DEV)
    view = buf[off:off + values.numel()]
    view.copy_(values)
    return buf, view


def _adamw_run(max_norm, seed=0, steps=4):
    """FusedAdamW on parameters, gradients and moments that are whole tensors or views starting 1, 2 or 3 elements into a
    buffer, next to torch.optim.AdamW (+ clip_grad_norm_) on aligned copies of the same values."""
    from future_od.optim import FusedAdamW
    g = torch.Generator().manual_seed(seed)
    ps_a, ps_b, bufs = [], [], []
    for n, po, go, mo, vo in LC.ADAMW_TENSORS:
        t = torch.randn(n, generator=g)
        buf, view = _offset_view(t, po)
        bufs.append((buf, po, n))
        ps_a.append(torch.nn.Parameter(view))
        ps_b.append(torch.nn.Parameter(t.clone().to(DEV)))
    a = FusedAdamW([{"params": ps_a[:4]}, {"params": ps_a[4:], "lr": 3e-4}], lr=1e-3, weight_decay=1e-2, max_norm=max_norm)
    b = torch.optim.AdamW([{"params": ps_b[:4]}, {"params": ps_b[4:], "lr": 3e-4}], lr=1e-3, weight_decay=1e-2)
    for p, (n, po, go, mo, vo) in zip(ps_a, LC.ADAMW_TENSORS):
        for key, off in (("exp_avg", mo), ("exp_avg_sq", vo)):
            buf, a.state[p][key] = _offset_view(torch.zeros(n), off)
            bufs.append((buf, off, n))
        assert (p.data_ptr() // 4 - po) % 4 == 0 and (a.state[p]["exp_avg"].data_ptr() // 4 - mo) % 4 == 0
    norms = []
    for step in range(steps):
        sq = 0.0
        for pa, pb, (n, po, go, mo, vo) in zip(ps_a, ps_b, LC.ADAMW_TENSORS):
            gr = torch.randn(n, generator=g)
            sq += float((gr.double() ** 2).sum())
            pa.grad, pb.grad = _offset_view(gr, go)[1], gr.clone().to(DEV)
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_(ps_b, max_norm)
        a.step(); b.step()
        norms.append((None if a.last_grad_norm is None else float(a.last_grad_norm.item()), sq))
    return a, ps_a, ps_b, norms, bufs, b


@pytest.mark.parametrize("max_norm", [0.1, 0.0])
def test_fused_adamw_unaligned_views_and_chunk_edges(max_norm):
    """test_fused_adamw_matches_torch with its bounds (rtol 2e-6, atol 2e-7 on parameters after 4 steps) at sizes on both
    sides of the 16384-element chunk, on the 16-byte path and on the scalar one ((p | g | m | v) & 15 != 0), with and
    without clipping.  The squared norm the clip reads, and fod_multi_sqnorm_acc on the same tables, against the float64
    norm at rtol 1e-5: f32 accumulation of at most 64 terms per thread, a tree and about 10 more additions stay below
    100 * 2^-24 relative on a sum of squares, and the square root halves it."""
    assert {t[0] for t in LC.ADAMW_TENSORS} == set(LC.ADAMW_SIZES)
    a, ps_a, ps_b, norms, bufs, b = _adamw_run(max_norm)
    for whole, off, n in bufs:                                       # parameters and both moments of every tensor
        assert bool((whole[:off] == LC.SENTINEL).all()) and bool((whole[off + n:] == LC.SENTINEL).all()), f"wrote outside a view of {n} at {off}"
    assert len(bufs) == 3 * len(ps_a)
    for pa, pb, t in zip(ps_a, ps_b, LC.ADAMW_TENSORS):
        torch.testing.assert_close(pa.detach(), pb.detach(), rtol=2e-6, atol=2e-7, msg=lambda m: f"{t}: {m}")
        # the kernel forms 1 - beta2 in f32 from the f32 beta2 (0.999f is off by up to 2^-25, i.e. 2^-25 / 1e-3 = 3e-5 of
        # 1 - beta2); torch forms it in double.  Twice that, for the rounding of the difference itself
        torch.testing.assert_close(a.state[pa]["exp_avg_sq"], b.state[pb]["exp_avg_sq"], rtol=6e-5, atol=1e-9)
    if max_norm > 0:
        for got_sq, want_sq in norms:
            assert abs(got_sq ** 0.5 - want_sq ** 0.5) <= 1e-5 * want_sq ** 0.5, (got_sq, want_sq)
    else:
        assert all(n[0] is None for n in norms)
    # the atomic form of the norm, on the tables of the plan the last step ran with (they name its gradients)
    ptrs, numel, _, bt, bc = a._plan["tab"]
    out = torch.zeros(1, device=DEV)
    L.call("fod_multi_sqnorm_acc", ops.ptr(ptrs), ops.ptr(numel), ops.ptr(bt), ops.ptr(bc), bt.numel(), ops.ptr(out), ops.stream())
    want = norms[-1][1] ** 0.5
    assert abs(float(out.item()) ** 0.5 - want) <= 1e-5 * want, (float(out.item()), norms[-1][1])


def test_fused_adamw_norm_is_bit_equal_in_deterministic_mode():
    """Two runs from equal inputs: the squared norms of every step and the parameters are bit-equal.  (The optimizer
    launches fod_multi_sqnorm_det whenever it clips, whatever the mode says: the switch is set because that is how a
    reproducible run is asked for, not because it selects the kernel.)"""
    Fn.set_deterministic(True)
    runs = [_adamw_run(0.1, seed=3, steps=2) for _ in range(2)]
    assert [n[0] for n in runs[0][3]] == [n[0] for n in runs[1][3]]
    for p0, p1 in zip(runs[0][1], runs[1][1]):
        assert torch.equal(p0.detach(), p1.detach())
