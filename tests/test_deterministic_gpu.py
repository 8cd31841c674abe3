"""Deterministic mode (Fn.set_deterministic / FOD_DETERMINISTIC=1): every gradient that the default path adds up with
f32 atomics is summed in a fixed order instead, so gradients, parameters and Adam moments are BIT-identical from run to
run on one GPU.  Bit equality below is torch.equal on every tensor: no tolerance, no tensor left out.

Per entry point: shapes of the headline workload (10 frames x 1450 tokens, D = 256, FFN 2048; ResNet-50 at 900 x 1600),
for which the launch geometry -- for the weight gradients: the route the library reports for the very call -- shows more
than one contributing workgroup per output element (otherwise a case shows nothing); three calls on the same operands, starting from zero and from a previous value; and
the deterministic result within the tolerance the entry's own test in test_kernels_gpu.py uses, against the default
form.  Then whole steps: small model eager / replayed / train mode with dropout, the real extent, two fresh processes."""
import contextlib
import hashlib
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"

if torch.cuda.is_available():
    from future_od.native import functional as Fn
    from future_od.native import lib as L
    from future_od.native import ops
    from future_od.native import wgrad
    from test_kernels_gpu import check, rnd


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


def _thrice(run):
    """run() -> tuple of output tensors; three calls, bit-equal."""
    outs = [tuple(t.clone() for t in run()) for _ in range(3)]
    torch.cuda.synchronize()
    for other in outs[1:]:
        assert len(other) == len(outs[0])
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b), float((a.float() - b.float()).abs().max())
    return outs[0]


def _default(run):
    ops.set_deterministic(False)
    out = tuple(t.clone() for t in run())
    ops.set_deterministic(True)
    return out


# ---- per entry point --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_gemm_tn_acc_det(dtype):
    M, N1, K2 = 14500, 2048, 256                  # the encoder's first feed-forward weight at 10 x 1450 tokens
    ops.set_deterministic(True)
    r = ops.gemm_tn_route(M, N1, K2, dtype, row_scale=True, colsum=True)
    assert (r.kernel, r.nsplit, r.uses_partials_ws) == (L.TN_128, 12, 1)     # 12 M-splits add into every dW / colsum element
    g, x = rnd((M, N1), dtype, 1).to(DEV), rnd((M, K2), dtype, 2).to(DEV)
    rs = (torch.rand(N1) + 0.5).to(DEV)
    dw0, cs0 = torch.randn(N1, K2, device=DEV), torch.randn(N1, device=DEV)
    for zeroed in (True, False):
        def run():
            dw = torch.zeros_like(dw0) if zeroed else dw0.clone()
            cs = torch.zeros_like(cs0) if zeroed else cs0.clone()
            ops.gemm_tn_acc(g, x, dw, row_scale=rs, colsum=cs, zeroed=zeroed)
            return dw, cs
        ops.set_deterministic(True)
        dw, cs = _thrice(run)
        dw_d, cs_d = _default(run)
        check(dw, dw_d, torch.float32 if dtype == torch.float32 else dtype, math.sqrt(M), f"gemm_tn_acc_det zeroed={zeroed}")
        check(cs, cs_d, torch.float32, math.sqrt(M), "gemm_tn_acc_det colsum")


def test_gemm_tn_acc_det_eight_wave_kernel(knobs):
    """The same entry through the 8-wave kernel (FOD_TN_BIG_DENSE=1): its fused bias gradient is added by several waves
    per workgroup and by every M-split."""
    knobs(FOD_TN_BIG_DENSE=1)
    M, N1, K2 = 14500, 2048, 256
    ops.set_deterministic(True)
    r = ops.gemm_tn_route(M, N1, K2, colsum=True)
    assert r.kernel == L.TN_BIG and r.nsplit > 1 and r.uses_partials_ws      # takes the 8-wave kernel, several M-splits
    dtype = torch.bfloat16
    g, x = rnd((M, N1), dtype, 3).to(DEV), rnd((M, K2), dtype, 4).to(DEV)
    dw0, cs0 = torch.randn(N1, K2, device=DEV), torch.randn(N1, device=DEV)
    for zeroed in (True, False):
        def run():
            dw = torch.zeros_like(dw0) if zeroed else dw0.clone()
            cs = torch.zeros_like(cs0) if zeroed else cs0.clone()
            ops.gemm_tn_acc(g, x, dw, colsum=cs, zeroed=zeroed)
            return dw, cs
        ops.set_deterministic(True)
        dw, cs = _thrice(run)
        dw_d, cs_d = _default(run)
        check(dw, dw_d, dtype, math.sqrt(M), f"gemm_tn_acc_det (8-wave) zeroed={zeroed}")
        check(cs, cs_d, torch.float32, math.sqrt(M), "gemm_tn_acc_det (8-wave) colsum")


def test_gemm_tn_multi_long_det():
    """One encoder layer's four long weight gradients (self-attention projections, the two feed-forward layers) at
    14 500 rows, through the queue's deterministic plan."""
    dtype = torch.bfloat16
    M = 14500
    cases = [(M, 512, 256), (M, 256, 256), (M, 2048, 256), (M, 256, 2048)]
    ops_in = [(rnd((m, n1), dtype, 70 + i).to(DEV), rnd((m, k2), dtype, 80 + i).to(DEV)) for i, (m, n1, k2) in enumerate(cases)]

    def flush(det, starts):
        ops.set_deterministic(det)
        q = Fn._WgradQueue()
        q.enabled = q.hold = q.long_enabled = True
        outs = []
        for (g, x), (dw0, db0) in zip(ops_in, starts):
            dw, db = dw0.clone(), db0.clone()
            q.tn(True, g, x, dw, db)
            outs += [dw, db]
        assert len(q.long_jobs) == len(cases)
        if det:
            assert all(wgrad.long_plan(m, q.long_rows, True)[1] > 1 for m, _, _ in cases)                    # several splits per element
            assert all(wgrad.long_plan(m, q.long_rows, True)[1] <= L.TN_DET_MAX_SPLITS for m, _, _ in cases)
        q.flush()
        assert q.launches == 1 and q.carried == len(cases)
        ops.set_deterministic(True)
        return tuple(outs)

    zeros = [(torch.zeros(n1, k2, device=DEV), torch.zeros(n1, device=DEV)) for _, n1, k2 in cases]
    prev = [(torch.randn(n1, k2, device=DEV), torch.randn(n1, device=DEV)) for _, n1, k2 in cases]
    for starts in (zeros, prev):
        got = _thrice(lambda: flush(True, starts))
        want = flush(False, starts)
        for i, (a, b) in enumerate(zip(got, want)):
            check(a, b, torch.float32, math.sqrt(M), f"tn multi long det vs default, output {i}")   # summation order only


CONVS = [   # (Nimg, H, W, Cin, Cout, k, stride, pad): ResNet-50 at 900 x 1600, 10 frames
    (10, 113, 200, 128, 128, 3, 1, 1),     # layer2 3x3
    (10, 57, 100, 1024, 256, 1, 1, 0),     # layer3 1x1
    (2, 29, 50, 512, 512, 3, 1, 1),        # layer4 3x3 on two frames: the 128 x 128 kernel (M < 8192)
]
CONV_KERNELS = ["TN_BIG", "TN_BIG", "TN_128"]


@pytest.mark.parametrize("case", CONVS)
def test_conv2d_wgrad_acc_det(case):
    n, h, w_, cin, cout, k, stride, pad = case
    dtype = torch.bfloat16
    geom = ops.conv_geom((n, h, w_, cin), cout, k, stride, pad)
    M = n * geom.Ho * geom.Wo
    ops.set_deterministic(True)
    r = ops.conv2d_route(L.CONV_WGRAD, geom)
    assert r.kernel == getattr(L, CONV_KERNELS[CONVS.index(case)]) and r.nsplit > 1 and r.uses_partials_ws
    x = rnd((n, h, w_, cin), dtype, 1).to(DEV)
    dy = rnd((n, geom.Ho, geom.Wo, cout), dtype, 4).to(DEV)
    rs = (torch.rand(cout) + 0.5).to(DEV)
    dw0 = torch.randn(cout, k, k, cin, device=DEV)
    for zeroed in (True, False):
        def run():
            dw = torch.zeros_like(dw0) if zeroed else dw0.clone()
            ops.conv2d_wgrad_acc(dy, x, dw, geom, row_scale=rs, zeroed=zeroed)
            return (dw,)
        ops.set_deterministic(True)
        (dw,) = _thrice(run)
        (dw_d,) = _default(run)
        check(dw, dw_d, dtype, math.sqrt(M), f"conv wgrad det {case} zeroed={zeroed}")


@pytest.mark.parametrize("rows,group_rows", [(14500, 0), (3072, 512)])
def test_layernorm_bwd_det(rows, group_rows):
    dtype, D = torch.bfloat16, 256
    groups = rows // group_rows if group_rows else 1
    # contributors per dgamma / dbeta element: workgroups (64 rows each per pass, at most 512) or the rows of a group
    assert (group_rows if group_rows else min(512, -(-rows // 64))) > 1
    dy, s = rnd((rows, D), dtype, 3).to(DEV), rnd((rows, D), dtype, 2).to(DEV)
    mean = s.float().mean(-1).contiguous()
    rstd = (s.float().var(-1, unbiased=False) + 1e-5).rsqrt().contiguous()
    gamma = (torch.rand(groups * D) + 0.5).to(DEV)
    dg0, db0 = torch.randn(groups * D, device=DEV), torch.randn(groups * D, device=DEV)
    for zeroed in (True, False):
        def run():
            dg = torch.zeros_like(dg0) if zeroed else dg0.clone()
            db = torch.zeros_like(db0) if zeroed else db0.clone()
            dx = ops.layernorm_bwd(dy, s, mean, rstd, gamma, dg, db, group_rows=group_rows)
            return dg, db, dx
        ops.set_deterministic(True)
        dg, db, dx = _thrice(run)
        dg_d, db_d, dx_d = _default(run)
        assert torch.equal(dx, dx_d)
        if group_rows:      # the bound of test_layernorm_grouped_parameter_tables
            assert torch.allclose(dg, dg_d, rtol=1e-5, atol=1e-5 * float(dg_d.abs().max()) + 1e-6)
            assert torch.allclose(db, db_d, rtol=1e-5, atol=1e-5 * float(db_d.abs().max()) + 1e-6)
        else:               # the bound of test_layernorm
            check(dg, dg_d, dtype, 8, "ln dgamma det")
            check(db, db_d, dtype, 8, "ln dbeta det")


@pytest.mark.parametrize("pre", [False, True])
def test_linear_add_norm_bwd_det(pre):
    dtype, M = torch.bfloat16, 256
    assert -(-M // 16) > 1                         # one workgroup per 16-row tile adds into every dgamma / dbeta element
    dy = rnd((M, 256), dtype, 51).to(DEV)
    s = rnd((M, 256), dtype, 52).to(DEV)
    gamma = (torch.rand(256) + 0.5).to(DEV)
    mean = s.float().mean(-1).contiguous()
    rstd = (s.float().var(-1, unbiased=False) + 1e-5).rsqrt().contiguous()
    wt = rnd((256, 256), dtype, 53, scale=1.0 / 16).to(DEV)
    pre_g = rnd((M, 256), dtype, 54).to(DEV) if pre else None
    pre_wt = rnd((256, 256), dtype, 55, scale=1.0 / 16).to(DEV) if pre else None
    dg0, db0 = torch.randn(256, device=DEV), torch.randn(256, device=DEV)
    for zeroed in (True, False):
        def run():
            dg = torch.zeros_like(dg0) if zeroed else dg0.clone()
            db = torch.zeros_like(db0) if zeroed else db0.clone()
            dsum, da = ops.linear_add_norm_bwd(dy, s, mean, rstd, gamma, wt, dg, db, pre_g=pre_g, pre_w_t=pre_wt)
            return dg, db, dsum, da
        ops.set_deterministic(True)
        dg, db, dsum, da = _thrice(run)
        dg_d, db_d, dsum_d, da_d = _default(run)
        assert torch.equal(dsum, dsum_d) and torch.equal(da, da_d)
        assert torch.allclose(dg, dg_d, rtol=1e-4, atol=1e-3) and torch.allclose(db, db_d, rtol=1e-4, atol=1e-3)


def test_mlp2_mul_bwd_det():
    dtype, M, Mq, D = torch.bfloat16, 256, 128, 256
    assert M // Mq > 1                             # two rows of the batch add into every element of the table's gradient
    dout, q, h = (rnd((M, D), dtype, 105 + i).to(DEV) for i in range(3))
    table = rnd((Mq, D), dtype, 104).to(DEV)
    w1t = rnd((D, D), dtype, 102, scale=1.0 / 16).to(DEV)
    w2t = rnd((D, D), dtype, 103, scale=1.0 / 16).to(DEV)
    dt0 = torch.randn(Mq, D, device=DEV)
    for zeroed in (True, False):
        def run():
            dtab = torch.zeros_like(dt0) if zeroed else dt0.clone()
            ds, dh, dx = ops.mlp2_mul_bwd(dout, table, q, h, w2t, w1t, dtab)
            return dtab, ds, dh, dx
        ops.set_deterministic(True)
        dtab, ds, dh, dx = _thrice(run)
        dtab_d, ds_d, dh_d, dx_d = _default(run)
        assert torch.equal(ds, ds_d) and torch.equal(dh, dh_d) and torch.equal(dx, dx_d)
        assert torch.allclose(dtab, dtab_d, rtol=1e-5, atol=1e-5 * float(dtab_d.abs().max()))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("group_rows", [0, 1450])
def test_colsum_acc_det(dtype, group_rows):
    M, N = 14500, 256
    groups = M // group_rows if group_rows else 1
    rows = group_rows or M
    splits = max(1, min(512 // (-(-N // 64) * groups), -(-rows // 64)))
    assert -(-rows // -(-rows // splits)) > 1      # row splits per output element
    g = rnd((M, N), dtype, 1).to(DEV)
    out0 = torch.randn(groups, N, device=DEV)
    for zeroed in (True, False):
        def run():
            out = torch.zeros_like(out0) if zeroed else out0.clone()
            ops.colsum_acc(g, out, group_rows=group_rows)
            return (out,)
        ops.set_deterministic(True)
        (out,) = _thrice(run)
        (out_d,) = _default(run)
        check(out, out_d, torch.float32, math.sqrt(M), "colsum det")


def test_default_mode_is_untouched_by_a_round_trip():
    """Off -> on -> off: the default form's outputs afterwards are what they were before, within its own tolerance (the
    atomics' order is free), and the switch reads off.  The mode leaves nothing behind."""
    dtype, M, N1, K2 = torch.bfloat16, 14500, 256, 256
    g, x = rnd((M, N1), dtype, 1).to(DEV), rnd((M, K2), dtype, 2).to(DEV)
    dy, s = rnd((M, 256), dtype, 3).to(DEV), rnd((M, 256), dtype, 4).to(DEV)
    mean = s.float().mean(-1).contiguous()
    rstd = (s.float().var(-1, unbiased=False) + 1e-5).rsqrt().contiguous()
    gamma = (torch.rand(256) + 0.5).to(DEV)

    def run():
        dw, cs = torch.zeros(N1, K2, device=DEV), torch.zeros(N1, device=DEV)
        ops.gemm_tn_acc(g, x, dw, colsum=cs, zeroed=True)
        dg, db = torch.zeros(256, device=DEV), torch.zeros(256, device=DEV)
        ops.layernorm_bwd(dy, s, mean, rstd, gamma, dg, db)
        return dw, cs, dg, db
    ops.set_deterministic(False)
    before = run()
    ops.set_deterministic(True)
    run()
    ops.set_deterministic(False)
    assert not ops.is_deterministic() and not Fn.is_deterministic()
    after = run()
    check(after[0], before[0], dtype, math.sqrt(M), "dw after the round trip")
    check(after[1], before[1], torch.float32, math.sqrt(M), "colsum after the round trip")
    check(after[2], before[2], dtype, 8, "dgamma after the round trip")
    check(after[3], before[3], dtype, 8, "dbeta after the round trip")


# ---- whole steps ------------------------------------------------------------------------------------------------------
def _state(model, opt):
    """Every gradient, parameter and Adam moment, by name."""
    out = {}
    for n, p in model.named_parameters():
        out["param " + n] = p.detach().clone()
        if p.grad is not None:
            out["grad " + n] = p.grad.detach().clone()
        st = opt.state.get(p, {})
        for k in ("exp_avg", "exp_avg_sq"):
            if k in st:
                out[f"{k} {n}"] = st[k].detach().clone()
    return out


def _assert_same_state(a, b, nparams):
    assert set(a) == set(b)
    count = {kind: sum(k.startswith(kind + " ") for k in a) for kind in ("param", "grad", "exp_avg", "exp_avg_sq")}
    print(f"compared {count} tensors ({nparams} parameters require a gradient)")
    assert count["param"] >= nparams and count["grad"] == count["exp_avg"] == count["exp_avg_sq"] == nparams, count
    bad = [k for k in a if not torch.equal(a[k], b[k])]
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("train_mode", [False, True])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_eager_steps_are_bit_reproducible(dtype, train_mode):
    from future_od.datasets.synthetic import make_batch
    from test_graph_gpu import _build, _eager_step
    ops.set_deterministic(True)
    data = make_batch(2, 3, 96, 128, seed=11, max_boxes=9, device=DEV)
    states = []
    for _ in range(2):
        model, opt = _build(dtype)
        if train_mode:
            model.train()
        Fn.manual_seed(0)
        for _ in range(5):
            _eager_step(model, opt, data)
        torch.cuda.synchronize()
        states.append(_state(model, opt))
        nparams = sum(1 for p in model.parameters() if p.requires_grad)
    _assert_same_state(states[0], states[1], nparams)


@pytest.mark.parametrize("train_mode", [False, True])
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_graph_replays_are_bit_reproducible(dtype, train_mode):
    from future_od.datasets.synthetic import make_batch
    from future_od.graph import GraphedStep
    from test_graph_gpu import _build
    ops.set_deterministic(True)
    data = make_batch(2, 3, 96, 128, seed=11, max_boxes=9, device=DEV)
    states = []
    for _ in range(2):
        model, opt = _build(dtype)
        if train_mode:
            model.train()
        Fn.manual_seed(0)
        step = GraphedStep(model, opt, warmup=2)
        for _ in range(5):
            step(data)
        torch.cuda.synchronize()
        assert step.replays == 5 and len(step._graphs) == 1
        states.append(_state(model, opt))
        nparams = sum(1 for p in model.parameters() if p.requires_grad)
    _assert_same_state(states[0], states[1], nparams)
    # the mode is part of what a graph was captured for: a flipped switch captures anew, it never replays this graph
    ops.set_deterministic(False)
    step(data)
    assert len(step._graphs) == 2
    ops.set_deterministic(True)
    step(data)
    assert len(step._graphs) == 2 and step.replays == 7


def _fullsize_grads(model, data, passes):
    runs = []
    for _ in range(passes):
        for p in model.parameters():
            p.grad = None
        _, _, loss, _, _ = model(data=data, distributed=False)
        loss.backward()
        torch.cuda.synchronize()
        runs.append({n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None})
    return runs


def test_real_extent_gradients_are_bit_reproducible():
    """B = 1, T = 6, 900 x 1600, ResNet-50, 6 + 6 layers, num_images = 5, bf16: three forward + backward passes from the
    same parameters.  Informative (printed, not asserted): how many gradient tensors differ between two passes with
    the mode OFF -- what the mode removes; were it 0, these shapes would show nothing."""
    from future_od.datasets.synthetic import make_batch
    from test_fullsize_oracle_gpu import CFG, H_, SEED, T_, W_
    from test_model_gpu import build_product
    model, _ = build_product(CFG, torch.bfloat16, SEED)
    data = make_batch(1, T_, H_, W_, seed=SEED, max_boxes=40, device=DEV)
    wanted = sum(1 for p in model.parameters() if p.requires_grad)
    ops.set_deterministic(True)
    runs = _fullsize_grads(model, data, 3)
    print(f"deterministic mode, real extent: {len(runs[0])} gradient tensors compared over 3 passes "
          f"({wanted} parameters require a gradient)")
    assert len(runs[0]) == wanted
    for other in runs[1:]:
        assert set(other) == set(runs[0])
        bad = [n for n in runs[0] if not torch.equal(runs[0][n], other[n])]
        assert not bad, (len(bad), bad[:8])
    ops.set_deterministic(False)
    off = _fullsize_grads(model, data, 2)
    differ = sum(1 for n in off[0] if not torch.equal(off[0][n], off[1][n]))
    print(f"default mode, real extent: {differ} of {len(off[0])} gradient tensors differ between two passes")


def _fresh_process(q):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "future-object-detection_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch as t
    from future_od.datasets.synthetic import make_batch
    from future_od.native import functional as F_
    from test_graph_gpu import _build, _eager_step
    t.cuda.set_device(0)
    F_.set_deterministic(True)
    F_.manual_seed(0)
    model, opt = _build("bf16")
    model.train()
    data = make_batch(2, 3, 96, 128, seed=11, max_boxes=9, device=DEV)
    for _ in range(3):
        _eager_step(model, opt, data)
    t.cuda.synchronize()
    h = hashlib.sha256()
    for _, p in sorted(model.named_parameters()):
        h.update(p.detach().cpu().contiguous().view(t.uint8).numpy().tobytes())
    q.put(h.hexdigest())


def test_two_fresh_processes_agree():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    digests = []
    for _ in range(2):                             # one after the other: one GPU
        q = ctx.Queue()
        p = ctx.Process(target=_fresh_process, args=(q,))
        p.start()
        digests.append(q.get(timeout=240))
        p.join(60)
        assert p.exitcode == 0
    assert digests[0] == digests[1], digests
