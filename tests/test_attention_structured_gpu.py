"""Every attention kernel against float64 on operands its roundings leave exact (tests/attention_cases.py).

With scale = ln(2) / 8 the kernels' c = scale * log2(e) is exactly 0.125 in f32, integer queries and keys give scores
that are exact multiples of 1/8 in every accumulator, and float64 softmax on the very same operands is the true answer
of what each kernel computes.  What is left is countable, in units of u = 2^-8 (bf16) relative to the SUM OF MAGNITUDES
`A` of an element's terms:

  o     the probability tile rounded to bf16 (attention.hip: frag_from_acc of sacc in attn_fwd_kernel / attn_fwd_lds_kernel),
        the normaliser summed from the same rounded tile in the LDS forward (the `fones` MFMA), the bf16 result: 3 u -> 4 u
  dv    P recomputed from the forward's lse2 and rounded, the result: 2 u -> 4 u
  dq*   P (through lse2), the dS tile rounded to bf16, delta = rowsum(dO * O) from the ROUNDED output, the product with
  dk*   the f32 scale, the result: 5 u -> 8 u
  lse2  2^-8 absolute in log2 units: a normaliser summed from bf16 probabilities moves it by log2(e) 2^-9, plus the f32 sum
  f32   2e-5 A (the rtol of test_kernels_gpu.tol), lse2 2^-10
  fp8   o within (2^-4 + 2^-6) A (P in e4m3), lse2 within 2^-3, gradients (bf16 kernels on the dequantised operands) as bf16
        plus what the backward inherits from the fp8 forward's lse2: probabilities below 2^-13 of the row's largest are
        rounded to e4m3's subnormal grid or flushed (attention_fp8.hip:28-29, the pack4(ex2f(..)) tile), so the normaliser
        misses up to their mass phi and every P of the backward is off by phi / (1 - phi) (attention_cases.fp8_backward_extra;
        the first run measured dv at 1.05 bounds at 128 x 1450 without this term: 1100 keys at 2^-16 of a pair)

Where A is 0 the result must be 0 (the flat profile's dk, the dq of a row without upstream gradient); no element is exempt.
A failure names the pass, the first bad (b, token, head, channel), the case and its route.  Each test prints its worst
err / bound per pass (pytest -s): lines `ATTN_RATIO|route|pass|ratio`."""
import contextlib

import pytest
import torch

import attention_cases as AC
import variant_cases as V
from future_od import switches

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

if torch.cuda.is_available():
    from future_od.native import functional as Fn
    from future_od.native import lib as L
    from future_od.native import ops

RUNS = AC.runs()
GRADS = ("dq1", "dk1", "dq2", "dk2", "dv")               # the order ops.attn_bwd returns them in


@pytest.fixture
def knobs():
    """knobs(FOD_X=v, ...): sets selection knobs of the library (csrc/knobs.h) for the rest of the test; the values
    they had come back at teardown."""
    with contextlib.ExitStack() as stack:
        yield lambda **values: stack.enter_context(L.knobs(**values))


def _dev(p, dtype):
    g = lambda t: None if t is None else t.to(dtype).to(DEV)
    return g(p.q1), g(p.k1), g(p.v), g(p.q2), g(p.k2), g(p.dout)


def _cpu(o, lse2, grads):
    got = dict(o=o.float().cpu(), lse2=lse2.float().cpu()) if lse2 is not None else dict(o=o.float().cpu())
    got.update({n: t.float().cpu() for n, t in zip(GRADS, grads) if t is not None})
    return got


def _report(route, worst):
    for name, ratio in worst.items():
        print(f"ATTN_RATIO|{route}|{name}|{ratio:.4f}")


def _merge(worst, more):
    for name, ratio in more.items():
        worst[name] = max(worst.get(name, 0.0), ratio)


def _tickets_are_zero(what):
    tickets = ops._attn_split_workspace(torch.device(DEV), 1)[1]
    assert int(tickets.abs().sum()) == 0, f"{what}: key-split tickets were not left at zero"


@pytest.mark.parametrize("c,profile", RUNS, ids=[AC.run_id(c, prof) for c, prof in RUNS])
def test_attention_on_exact_operands(knobs, c, profile):
    """ops.attn_fwd, then ops.attn_bwd consuming the forward's own o and lse2 (as the model does), every call of the case,
    under the case's knobs, the route asked first.  Key-split cases: every call twice on one stream, equal results and
    the tickets back at zero."""
    knobs(**c.knobs)
    r = V.assert_route(c)
    dtype = V.DTYPE[c.dtype]
    route = AC.route_name(c)
    what = f"{AC.run_id(c, profile)} ({route})"
    twice = c.expect.get("ksplit", 1) > 1
    assert twice == (r.ksplit > 1)
    worst = {}
    for call in range(AC.n_calls(c.shape, profile)):
        p = AC.problem(c.shape, profile, call)
        q1, k1, v, q2, k2, dout = _dev(p, dtype)
        kw = dict(drop_p=p.drop, drop_seed=p.seed) if p.drop else {}
        results = []
        for _ in range(2 if twice else 1):
            o, lse2 = ops.attn_fwd(q1, k1, v, AC.SCALE, q2, k2, **kw)
            results.append((o, lse2, ops.attn_bwd(q1, k1, v, o, dout, lse2, AC.SCALE, q2, k2, **kw)))
        o, lse2, grads = results[0]
        _merge(worst, AC.assert_within(p, _cpu(o, lse2, grads), c.dtype, what))
        if twice:
            o_b, lse2_b, grads_b = results[1]
            assert torch.equal(o, o_b) and torch.equal(lse2, lse2_b), f"{what} call {call}: the second forward differs"
            for name, a, b in zip(GRADS, grads, grads_b):
                assert a is None or torch.equal(a, b), f"{what} call {call}: the second {name} differs"
    if twice:
        _tickets_are_zero(what)
    _report(route, worst)


# ------------------------------------------------------------------------------------------------ the queued dk / dv pass
DKV_SHAPE = (2, 2, 64, 300)                               # Tq <= 512, S >= 256: what the model queues; S % 128 != 0


@pytest.mark.parametrize("parts", [1, 2])
@pytest.mark.parametrize("njobs", [3, 32])
def test_dkv_multi_jobs_against_their_own_references(njobs, parts):
    """ops.attn_bwd_dq + ops.attn_bwd_dkv_multi called directly: 3 and 32 (DKV_MAX_JOBS) jobs of B = 2, every job with
    operands of its own (another call index of the pointer profile, which moves keys, values, targets and dout).  Each
    job's dk1 / dk2 / dv is held to its own float64 reference, and is bit-equal to ops.attn_bwd's for the same job: the
    route's dk / dv kernel is the prefetching one, whose body the queue promises to run."""
    shape = DKV_SHAPE + (parts,)
    r = ops.attn_route(*shape)
    assert r.dkv == L.ATTN_PREFETCH and r.key_split == 1
    two = parts == 2
    jobs, keep, shp = [], [], None
    for j in range(njobs):
        p = AC.problem(shape, "pointer", j)
        q1, k1, v, q2, k2, dout = _dev(p, torch.bfloat16)
        o, lse2 = ops.attn_fwd(q1, k1, v, AC.SCALE, q2, k2)
        whole = ops.attn_bwd(q1, k1, v, o, dout, lse2, AC.SCALE, q2, k2)
        dk1, dv = torch.full_like(k1, float("nan")), torch.full_like(v, float("nan"))
        dk2 = torch.full_like(k2, float("nan")) if two else None
        dq1, dq2, delta, shp = ops.attn_bwd_dq(q1, k1, v, o, dout, lse2, AC.SCALE, q2, k2, dk2_like=dk2)
        jobs.append((q1, q2, k1, k2, v, dout, lse2, delta, dk1, dk2, dv))
        keep.append((p, o, lse2, whole, dq1, dq2))
    ops.attn_bwd_dkv_multi(jobs, shp)
    worst = {}
    for j, (job, (p, o, lse2, whole, dq1, dq2)) in enumerate(zip(jobs, keep)):
        dk1, dk2, dv = job[8], job[9], job[10]
        what = f"dkv_multi job {j} of {njobs}, shape {shape}"
        _merge(worst, AC.assert_within(p, _cpu(o, lse2, (dq1, dk1, dq2, dk2, dv)), "bf16", what))
        for name, mine, theirs in zip(GRADS, (dq1, dk1, dq2, dk2, dv), whole):
            assert mine is None or torch.equal(mine, theirs), f"{what}: {name} differs from ops.attn_bwd's"
    _tickets_are_zero(f"dkv_multi {shape}")
    _report(f"bf16:dkv_multi{njobs}", worst)


# ------------------------------------------------------------------------------------------------ the fp8 forward
FP8_RUNS = [(s, prof, st) for s in AC.fp8_shapes() for prof in ("pointer", "flat") for st in (None, 2)]


@pytest.mark.parametrize("shape,profile,stage", FP8_RUNS,
                         ids=["x".join(map(str, s)) + f"-{prof}-stage{st or 'default'}" for s, prof, st in FP8_RUNS])
def test_fp8_forward_on_exact_operands(knobs, shape, profile, stage):
    """ops.attn_fwd_fp8 on operands MX e4m3 holds exactly: the dequantised copies ARE the operands (q times 0.125), bit for
    bit; o within (2^-4 + 2^-6) A_o, lse2 within 2^-3; then the bf16 backward on the copies (scale 1 / log2 e, dq scaled by
    0.125) under the bf16 gradient bounds plus the flushed-probability term of the module docstring.  By default and with
    two key tiles per barrier (FOD_FP8_STAGE=2)."""
    if stage is not None:
        knobs(FOD_FP8_STAGE=stage)
        assert L.knob("FOD_FP8_STAGE") == str(stage)
    worst = {}
    for call in range(min(AC.n_calls(shape, profile), 4)):
        p = AC.problem(shape, profile, call)
        what = f"fp8 {shape} {profile} stage {stage}"
        q1, k1, v, q2, k2, dout = _dev(p, torch.bfloat16)
        o, lse2, deq = ops.attn_fwd_fp8(q1, k1, v, AC.SCALE, q2, k2, want_backward=True)
        for name, got, want in zip(("q1", "k1", "v", "q2", "k2"), deq, (q1 * 0.125, k1, v, None if q2 is None else q2 * 0.125, k2)):
            assert want is None or torch.equal(got, want), f"{what} call {call}: dequantised {name} is not the operand"
        _merge(worst, AC.assert_within(p, _cpu(o, lse2, ()), "bf16", what, factors=AC.FP8_FACTOR, passes=("o", "lse2")))
        grads = ops.attn_bwd(deq[0], deq[1], deq[2], o, dout, lse2, 1.0 / ops.LOG2E, deq[3], deq[4], dq_scale=0.125)
        got = _cpu(o, None, grads)
        _merge(worst, AC.assert_within(p, got, "bf16", what, passes=[n for n in GRADS if n in got], extra=AC.fp8_backward_extra(p)))
    _report(f"fp8:stage{stage or 'default'}", worst)


# ------------------------------------------------------------------------------------------------ through autograd
CROSS = (2, 8, 128, 1450, 2)


def _leaves(p):
    return [t.requires_grad_(True) for t in _dev(p, torch.bfloat16)[:5]]


def test_autograd_node_on_the_cross_attention_shape():
    """Fn.attention on the two-part cross-attention shape with FOD_DKV_QUEUE on: the autograd node's pointer plumbing
    under the same bounds."""
    worst = {}
    with switches.override(FOD_DKV_QUEUE=True):
        for call in (0, 1):
            p = AC.problem(CROSS, "pointer", call)
            q1, k1, v, q2, k2 = _leaves(p)
            o = Fn.attention(q1, k1, v, AC.SCALE, q2, k2)
            o.backward(p.dout.to(torch.bfloat16).to(DEV))
            got = _cpu(o.detach(), None, (q1.grad, k1.grad, q2.grad, k2.grad, v.grad))
            _merge(worst, AC.assert_within(p, got, "bf16", f"Fn.attention {CROSS}", passes=["o"] + list(GRADS)))
    _report("bf16:Fn.attention", worst)


def test_hoisted_cross_attention_queues_its_key_value_pass():
    """Fn.hoisted_cross_attention (the decoder's node: k / v as column slots of the hoisted buffers, the dk / dv pass queued
    and run by fod_attn_bwd_dkv_multi when layer 0 hands the buffers on) with FOD_DKV_QUEUE on and off: the gradients of
    the buffers under the same bounds."""
    B, H, Tq, S, parts = CROSS
    D = H * 32
    for queued in (True, False):
        worst = {}
        with switches.override(FOD_DKV_QUEUE=queued):
            p = AC.problem(CROSS, "pointer", 1)
            q1, k1, v, q2, k2 = _dev(p, torch.bfloat16)[:5]
            q1.requires_grad_(True), q2.requires_grad_(True)
            big = torch.cat([v, k1], dim=-1).contiguous().requires_grad_(True)        # per layer: [value | key_content]
            ks_all = k2.clone().requires_grad_(True)                                   # per-batch position keys
            side = Fn.MemorySide([big], ks_all, 1, 1, D)
            o = Fn.hoisted_cross_attention(q1, q2, side, 0, 0, AC.SCALE)
            o.backward(p.dout.to(torch.bfloat16).to(DEV))
            got = _cpu(o.detach(), None, (q1.grad, big.grad[..., D:], q2.grad, ks_all.grad, big.grad[..., :D]))
            _merge(worst, AC.assert_within(p, got, "bf16", f"hoisted cross-attention {CROSS} queued={queued}",
                                           passes=["o"] + list(GRADS)))
        _report(f"bf16:hoisted-queue{int(queued)}", worst)
