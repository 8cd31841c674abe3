"""Every autograd node of future_od/native/functional.py against float64 torch autograd on the CPU.

The kernels are held against float64 torch in test_kernels_gpu.py, test_variants_gpu.py and test_layout_gpu.py; this file
checks what the Functions' backward methods do ON TOP of them -- slicing packed weights, summing periodic rows, routing
gradients into the slots of shared buffers, deferring sums to queues, deciding which call hands a total on -- against an
oracle that shares no code with them.

One method for every case (tests/autograd_node_cases.py lists them per node):
  * inputs, parameters and incoming gradients come from seeded CPU generators and are rounded to the case's dtype;
  * the node runs on the GPU through its public wrapper, backward from sum((out.float() * gout.float()).sum());
  * the reference is the same mathematics in plain torch ops in float64 on the CPU, from the same rounded values,
    differentiated by torch autograd; nothing of future_od or oracle/ is used in it;
  * compared: the forward outputs and EVERY gradient (inputs, tables, each parameter), as ||got - ref|| / ||ref|| per
    SLICE (each third of a packed in_proj weight, each column slot of a hoisted buffer, ...): one wrong row or one
    swapped slice moves that ratio to order 1 at these sizes.  A gradient must exist and have its tensor's shape; where the
    reference is exactly zero it must be exactly zero (a parameter no output depends on may go without one, unless the
    case is about explicit zeros).  The bias of a softmax's keys has no gradient in exact arithmetic -- the column sums
    of dk cancel -- and is measured against the column sums of |dk| instead of against its own (zero) norm.
Every case runs with the weight-gradient queue off, with it on, and in deterministic mode, under the same limits:
autograd_node_cases.LIMIT for a single node, three times a CPU-measured figure for a chain of nodes (Case.measured).

`python tests/test_autograd_nodes_gpu.py` prints those figures; it needs no GPU.
"""
import functools
import math
import sys
import zlib
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import autograd_node_cases as NC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
MODES = ("off", "queue", "det")          # the weight-gradient queue off / on (eager), deterministic mode
D = 256                                  # the fused kernels' width: 8 heads of 32


# ------------------------------------------------------------------------------------------------ tensors of a case
class Spec:
    def __init__(self, shape, kind, scale, mean, grad, f32):
        self.shape, self.kind, self.scale, self.mean, self.grad, self.f32 = tuple(shape), kind, scale, mean, grad, f32


def A(*shape, s=1.0, grad=True, f32=False, mean=0.0):
    """An activation: stored in the compute dtype (f32=True: float32 whatever the compute dtype)."""
    return Spec(shape, "act", s, mean, grad, f32)


def P(*shape, s=1.0, mean=0.0):
    """A parameter: a float32 leaf whose values are representable in the compute dtype."""
    return Spec(shape, "param", s, mean, True, True)


def W(n=D, k=D):
    return P(n, k, s=1.0 / math.sqrt(k))


def B_(n=D):
    return P(n, s=0.3)


def GAMMA():
    return P(D, s=0.2, mean=1.0)


class NS(dict):
    __getattr__ = dict.__getitem__


def _values(case, dtype):
    """name -> float32 CPU tensor holding values rounded to `dtype`."""
    out = {}
    for name, sp in case.T.items():
        g = torch.Generator().manual_seed(zlib.crc32(f"{case.__name__}/{name}".encode()))
        out[name] = (torch.randn(sp.shape, generator=g) * sp.scale + sp.mean).to(dtype).float()
    return out


def _gout(case, name, shape, dtype):
    g = torch.Generator().manual_seed(zlib.crc32(f"{case.__name__}/gout/{name}".encode()))
    return torch.randn(tuple(shape), generator=g).to(dtype).float()


def _split(res):
    res = dict(res)
    keep = res.pop("_keep", {})
    after = res.pop("_after", None)
    mass = res.pop("_mass", {})
    return res, keep, after, mass


def cols(n, size, label):
    return [(f"{label}{i}", (Ellipsis, slice(i * size, (i + 1) * size))) for i in range(n)]


THIRDS = [(n, (slice(i * D, (i + 1) * D),)) for i, n in enumerate("qkv")]      # a packed in_proj weight / bias
WHOLE = [("", (Ellipsis,))]


# ------------------------------------------------------------------------------------------------ the float64 side
def lin(x, w, b=None):
    return F.linear(x, w, b)


def ln(x, g, b):
    return F.layer_norm(x, (x.shape[-1],), g, b, 1e-5)


def attn(q1, k1, v, scale, q2=None, k2=None):
    """softmax((q1.k1 + q2.k2) * scale) v per head, heads of 32 columns per part."""
    Bq, T_, E = q1.shape
    H = E // 32
    heads = lambda t: t.reshape(t.shape[0], t.shape[1], H, 32).transpose(1, 2)
    s = heads(q1) @ heads(k1).transpose(-1, -2)
    if q2 is not None:
        s = s + heads(q2) @ heads(k2).transpose(-1, -2)
    p = torch.softmax(s * scale, dim=-1)
    return (p @ heads(v)).transpose(1, 2).reshape(Bq, T_, E)


def _ident(x):
    return x


def _bf16(x):
    """A bf16 store: the value is rounded, and so is the gradient that comes back through it."""
    return x.to(torch.bfloat16).double()


def run_ref(case, dtype_name, rounded=False):
    """(outputs, gradients of the leaves, gradients of the kept intermediates) in float64 on the CPU.  `rounded`: the
    reference with a bf16 rounding at every tensor the nodes store -- what Case.measured is measured with."""
    dtype = DT[dtype_name]
    r = _bf16 if rounded else _ident
    leaves, t = {}, NS()
    for name, v in _values(case, dtype).items():
        sp = case.T[name]
        leaves[name] = v.double().requires_grad_(sp.grad)
        t[name] = r(leaves[name]) if (sp.kind == "act" and not sp.f32) else leaves[name]
    outs, keep, _, mass = _split(case.ref(t, r))
    for k in list(keep.values()) + list(mass.values()):
        k.retain_grad()
    loss = sum((o * _gout(case, n, o.shape, dtype).double()).sum() for n, o in outs.items())
    loss.backward()
    grads = {n: (None if not case.T[n].grad else (torch.zeros_like(l) if l.grad is None else l.grad))
             for n, l in leaves.items()}
    # a bias that is added to every key of a softmax has no gradient: the column sums of dk cancel.  Such a slice is
    # measured against what the sum would be WITHOUT cancellation -- the norm of the column sums of |dk| -- as
    # test_colsum_groups_multi bounds its sums by their mass
    scales = {key: float(k.grad.abs().reshape(-1, k.shape[-1]).sum(0).norm()) for key, k in mass.items()}
    return ({n: o.detach() for n, o in outs.items()}, grads, {n: k.grad for n, k in keep.items()}, scales)


@functools.lru_cache(maxsize=None)
def reference(case_name, dtype_name):
    """Computed once per (case, dtype) and shared by the three modes; never modified."""
    return run_ref(CASES[case_name], dtype_name)


# ------------------------------------------------------------------------------------------------ the GPU side
def run_gpu(case, dtype_name, mode):
    from future_od import switches
    from future_od.native import functional as Fn
    from future_od.native import ops
    dtype = DT[dtype_name]
    leaves = NS()
    for name, v in _values(case, dtype).items():
        sp = case.T[name]
        if sp.kind == "param":
            leaves[name] = torch.nn.Parameter(v.to(DEV))
        else:
            leaves[name] = v.to(torch.float32 if sp.f32 else dtype).to(DEV).requires_grad_(sp.grad)
    t = NS(leaves)
    t["dtype"], t["mode"] = dtype, mode
    q = Fn.WGRADS
    was, det_was = (q.enabled, q.eager), ops.is_deterministic()
    try:
        q.enabled = q.eager = mode == "queue"            # (outside a capture the queue is off unless asked for)
        ops.set_deterministic(mode == "det")
        with switches.override(FOD_ATTN_FP8="off", **getattr(case, "SWITCHES", {})):
            Fn.PREP.clear()
            t["launches"], t["carried"] = q.launches, q.carried
            outs, keep, after, _ = _split(case.gpu(t, Fn))
            for k in keep.values():
                k.retain_grad()
            loss = sum((o.float() * _gout(case, n, o.shape, dtype).to(DEV).float()).sum() for n, o in outs.items())
            loss.backward()
            torch.cuda.synchronize()
            if after is not None:
                after(t, Fn)
    finally:
        q.enabled, q.eager = was
        ops.set_deterministic(det_was)
    grads = {n: leaves[n].grad for n in case.T}
    return ({n: o.detach() for n, o in outs.items()}, grads, {n: k.grad for n, k in keep.items()})


def _compare(kind, tensor, got, ref, slices, limit_of, bad, figures, scales=None):
    """kind: "out" | "d" (a gradient); `limit_of(slice name)`; `scales`: {(tensor, slice label): norm} for the slices
    that cancel to zero in exact arithmetic (see run_ref)."""
    what = f"{kind} {tensor}"
    if got is None:
        bad.append(f"{what}: no gradient")
        return
    if tuple(got.shape) != tuple(ref.shape):
        bad.append(f"{what}: shape {tuple(got.shape)}, expected {tuple(ref.shape)}")
        return
    got = got.detach().double().cpu()
    for label, idx in slices:
        g, w = got[idx], ref[idx]
        name = what + (f"[{label}]" if label else "")
        den = (scales or {}).get((tensor, label), float(w.norm()))
        if den == 0.0:
            if float(g.abs().max()) != 0.0:
                bad.append(f"{name}: reference exactly zero, got max |x| = {float(g.abs().max()):.3e}")
            figures.append((name, 0.0))
            continue
        err = float((g - w).norm()) / den
        figures.append((name, err))
        if not err <= limit_of(name):
            bad.append(f"{name}: {err:.3e} > {limit_of(name):.3e}")


def _all_cases():
    return [(name, dt, mode) for name, c in NC.CASES.items() for dt in c.dtypes for mode in MODES]


@pytest.mark.parametrize("name,dtype_name,mode", _all_cases(), ids=lambda v: str(v))
def test_node_against_float64_autograd(name, dtype_name, mode):
    case = CASES[name]
    limit = lambda what: NC.limit(name, dtype_name, what)
    ref_out, ref_grad, ref_keep, scales = reference(name, dtype_name)
    out, grad, keep = run_gpu(case, dtype_name, mode)
    bad, figures = [], []
    slices = getattr(case, "S", {})
    assert out.keys() == ref_out.keys()
    for n in ref_out:
        _compare("out", n, out[n], ref_out[n], slices.get(n, WHOLE), limit, bad, figures)
    for n, w in ref_grad.items():
        if w is None:
            if grad[n] is not None:
                bad.append(f"d {n}: a gradient for an input that asked for none")
            continue
        if grad[n] is None and float(w.abs().max()) == 0.0 and n not in getattr(case, "EXPLICIT_ZEROS", ()):
            continue         # a parameter no output depends on: no gradient is a zero gradient (an explicit one is checked)
        _compare("d", n, grad[n], w, slices.get(n, WHOLE), limit, bad, figures, scales)
    assert keep.keys() == ref_keep.keys()
    for n in ref_keep:
        _compare("d", n, keep[n], ref_keep[n], slices.get(n, WHOLE), limit, bad, figures)
    worst = max(figures, key=lambda f: f[1] / limit(f[0]))
    print(f"{name} {dtype_name} {mode}: limit {limit(worst[0]):.2e}, worst {worst[1]:.3e} at {worst[0]}; "
          + ", ".join(f"{n} {e:.2e}" for n, e in figures))
    assert not bad, f"{name} {dtype_name} {mode}:\n  " + "\n  ".join(bad)


def test_every_case_of_the_table_is_defined():
    assert set(CASES) == set(NC.CASES), sorted(set(CASES) ^ set(NC.CASES))


@pytest.mark.parametrize("dtype_name", NC.BOTH)
def test_group_linear_refuses_a_table_longer_than_its_period(dtype_name):
    """group_linear(residual=..., res_row_mod=m): a table has exactly m rows (the decoder's query positions are the only
    caller).  With more, GroupLinearFn.backward and the AddFn fallback would view an [m, D] sum as the table's shape."""
    from future_od.native import functional as Fn
    dtype = DT[dtype_name]
    x = torch.zeros(2, 20, D, dtype=dtype, device=DEV)
    lins = [Lin(torch.nn.Parameter(torch.zeros(D, D, device=DEV)), torch.nn.Parameter(torch.zeros(D, device=DEV))) for _ in range(3)]
    tabs = torch.zeros(2, 40, D, dtype=dtype, device=DEV, requires_grad=True)
    with pytest.raises(AssertionError, match="res_row_mod"):
        Fn.group_linear(x, lins, residual=[tabs[0], tabs[1]], res_row_mod=20)


# ------------------------------------------------------------------------------------------------ the cases
CASES = {}


def case(cls):
    CASES[cls.__name__] = cls
    return cls


def Lin(w, b):
    return SimpleNamespace(weight=w, bias=b)


def _queued(t, Fn, jobs):
    """bf16 with the queue on: `jobs` weight-gradient jobs of this pass went through one multi launch."""
    if t.mode == "queue" and t.dtype == torch.bfloat16:
        got = (Fn.WGRADS.launches - t.launches, Fn.WGRADS.carried - t.carried)
        assert got == (1, jobs), got


# -- LinearFn
class _Linear:
    T = dict(x=A(2, 20, D), w=W(), b=B_())
    relu, out_f32, jobs = False, False, 1

    @classmethod
    def gpu(cls, t, Fn):
        return dict(y=Fn.linear(t.x, t.w, t.b, relu=cls.relu, out_f32=cls.out_f32),
                    _after=lambda t, Fn: _queued(t, Fn, cls.jobs))

    @classmethod
    def ref(cls, t, r):
        y = lin(t.x, t.w, t.b)
        return dict(y=F.relu(y) if cls.relu else y)


@case
class linear_plain(_Linear):
    pass


@case
class linear_relu(_Linear):
    relu = True


@case
class linear_out_f32(_Linear):
    T = dict(x=A(2, 20, D), w=W(64), b=B_(64))
    out_f32 = True


@case
class linear_n2(_Linear):
    T = dict(x=A(2, 20, D), w=W(2), b=B_(2))

    @classmethod
    def gpu(cls, t, Fn):
        return dict(y=Fn.linear(t.x, t.w, t.b))


@case
class linear_shared_twice:
    T = dict(x1=A(2, 20, D), x2=A(23, D), w=W(), b=B_())

    def gpu(t, Fn):
        # the second use runs first in the backward pass and owns the job; the first use joins it (WGRADS.chain)
        return dict(y1=Fn.linear(t.x1, t.w, t.b), y2=Fn.linear(t.x2, t.w, t.b), _after=lambda t, Fn: _queued(t, Fn, 2))

    def ref(t, r):
        return dict(y1=lin(t.x1, t.w, t.b), y2=lin(t.x2, t.w, t.b))


# -- LinearKeepFn
class _Keep:
    T = dict(x=A(2, 20, D), w=W(), b=B_())
    relu = False

    @classmethod
    def gpu(cls, t, Fn):
        xk, y = Fn.linear_keep(t.x, t.w, t.b, relu=cls.relu)
        assert (xk is not t.x) == (t.w.shape[0] % 8 == 0)        # LinearKeepFn, or the two-consumer fallback
        return dict(xk=xk, y=y)

    @classmethod
    def ref(cls, t, r):
        y = lin(t.x, t.w, t.b)
        return dict(xk=t.x * 1.0, y=F.relu(y) if cls.relu else y)


@case
class keep_plain(_Keep):
    pass


@case
class keep_relu(_Keep):
    relu = True


@case
class keep_fallback_n2(_Keep):
    T = dict(x=A(2, 20, D), w=W(2), b=B_(2))


@case
class ffn_masked_tail:
    """The feed-forward block: the ReLU's producer leaves the gradient mask to the fused tail."""
    T = dict(x=A(2, 20, D), w0=W(512, D), b0=B_(512), w3=W(D, 512), b3=B_(), g=GAMMA(), be=B_())

    def gpu(t, Fn):
        xk, h = Fn.linear_keep(t.x, t.w0, t.b0, relu=True, grad_masked=True)
        assert xk is not t.x
        return dict(y=Fn.linear_add_norm(h, xk, t.w3, t.b3, t.g, t.be, a_relu=True))

    def ref(t, r):
        h = r(F.relu(lin(t.x, t.w0, t.b0)))
        o = r(lin(h, t.w3, t.b3))
        s = r(t.x + o)
        return dict(y=r(ln(s, t.g, t.be)))


# -- AddFn, MulFn, ExpandRowsFn, CastFn, ZeroGradAnchor
@case
class add_same:
    T = dict(a=A(2, 20, D), b=A(2, 20, D))

    def gpu(t, Fn):
        return dict(y=Fn.add(t.a, t.b))

    def ref(t, r):
        return dict(y=t.a + t.b)


@case
class add_row_mod:
    T = dict(a=A(2, 20, D), b=A(20, D))

    def gpu(t, Fn):
        return dict(y=Fn.add(t.a, t.b, b_row_mod=20))

    def ref(t, r):
        return dict(y=t.a + t.b.repeat(2, 1).view(2, 20, D))


@case
class add_row_div:
    T = dict(a=A(3, 42, D), b=A(3, D))

    def gpu(t, Fn):
        return dict(y=Fn.add(t.a, t.b, b_row_div=42))

    def ref(t, r):
        return dict(y=t.a + t.b.repeat_interleave(42, 0).view(3, 42, D))


@case
class mul_same:
    T = dict(a=A(40, D), b=A(40, D))

    def gpu(t, Fn):
        return dict(y=Fn.mul(t.a, t.b))

    def ref(t, r):
        return dict(y=t.a * t.b)


@case
class mul_row_mod:
    T = dict(a=A(60, D), b=A(20, D))

    def gpu(t, Fn):
        return dict(y=Fn.mul(t.a, t.b, b_row_mod=20))

    def ref(t, r):
        return dict(y=t.a * t.b.repeat(3, 1))


@case
class expand_rows3:
    T = dict(x=A(20, D))

    def gpu(t, Fn):
        return dict(y=Fn.expand_rows(t.x, 3))

    def ref(t, r):
        return dict(y=t.x.repeat(3, 1))


@case
class cast_pad:
    T = dict(x=A(2, 20, 2, f32=True))

    def gpu(t, Fn):
        y = Fn.cast_ad(t.x, t.dtype, pad_cols=8)
        assert y.dtype == t.dtype and y.grad_fn is not None
        return dict(y=y)

    def ref(t, r):
        return dict(y=F.pad(t.x, (0, 6)))


@case
class cast_noop:
    T = dict(x=A(2, 20, D))

    def gpu(t, Fn):
        assert Fn.cast_ad(t.x, t.dtype) is t.x and Fn.cast_ad(t.x, t.dtype, pad_cols=D) is t.x
        return dict(y=Fn.cast_ad(t.x, t.dtype))

    def ref(t, r):
        return dict(y=t.x)


@case
class zero_grad_anchor:
    """Identity on x; the listed parameters get explicit zeros (the reference leaves them without a gradient: zero)."""
    T = dict(x=A(2, 20, D), w=W(), b=B_(), w2=W(64, D))
    EXPLICIT_ZEROS = ("w", "b", "w2")

    def gpu(t, Fn):
        return dict(y=Fn.ZeroGradAnchor.apply(t.x, t.w, t.b, t.w2))

    def ref(t, r):
        return dict(y=t.x * 1.0)


# -- RefPointSineFn, BoxFinishFn (no wrappers: the models apply them directly)
def sine_embed(ref, width):
    """ref [R, 2] = (x, y) in (0, 1) -> [R, width] ordered (y | x): sin / cos pairs of 2 pi p / 10000^(2 (i // 2) / (width / 2))."""
    i = torch.arange(width // 2, dtype=torch.float64)
    dim_t = 10000.0 ** (2 * torch.div(i, 2, rounding_mode="floor") / (width // 2))

    def half(p):
        a = p[:, None] * (2 * math.pi) / dim_t
        return torch.stack((a[:, 0::2].sin(), a[:, 1::2].cos()), dim=2).flatten(1)

    return torch.cat((half(ref[:, 1]), half(ref[:, 0])), dim=1)


def logit_of(p):
    return torch.log(p / (1 - p))


def finish_boxes(t, ref):
    """sigmoid(t + [logit(ref[r % rows(ref)]), 0, 0]) for t [Lv, R, 4]."""
    rl = logit_of(ref).repeat(t.shape[1] // ref.shape[0], 1)
    return torch.cat([t[..., :2] + rl, t[..., 2:]], -1).sigmoid()


class _RefPoint:
    T = dict(logit=A(20, 2))
    use = ("ref", "sine")

    @classmethod
    def gpu(cls, t, Fn):
        ref, sine = Fn.RefPointSineFn.apply(t.logit, D)
        assert ref.dtype == torch.float32 and sine.dtype == t.dtype
        return {n: v for n, v in (("ref", ref), ("sine", sine)) if n in cls.use}

    @classmethod
    def ref(cls, t, r):
        ref = t.logit.sigmoid()
        return {n: v for n, v in (("ref", ref), ("sine", sine_embed(ref, D))) if n in cls.use}


@case
class refpoint_both(_RefPoint):
    pass


@case
class refpoint_ref_only(_RefPoint):
    use = ("ref",)


@case
class refpoint_sine_only(_RefPoint):
    use = ("sine",)


@case
class box_finish_shared_points:
    """The box head as paper.py applies it: t of all levels as [Lv, B * M, 4], the M reference points shared by the batch."""
    T = dict(t=A(3, 40, 4), ref=A(20, 2, s=0.15, mean=0.5, f32=True))

    def gpu(t, Fn):
        return dict(boxes=Fn.BoxFinishFn.apply(t.t, t.ref, 3))

    def ref(t, r):
        return dict(boxes=finish_boxes(t.t, t.ref))


@case
class refpoint_into_boxes:
    """Both nodes as the decoder and the box head chain them: the reference points' gradient from the boxes of every level
    and batch row returns to RefPointSineFn as dref beside dsine.  t is handed over 4-D and viewed, as the model does."""
    T = dict(logit=A(20, 2), t=A(3, 2, 20, 4))

    def gpu(t, Fn):
        ref, sine = Fn.RefPointSineFn.apply(t.logit, D)
        return dict(sine=sine, boxes=Fn.BoxFinishFn.apply(t.t.view(3, 40, 4), ref, 3).view(3, 2, 20, 4))

    def ref(t, r):
        ref = t.logit.sigmoid()
        return dict(sine=sine_embed(ref, D), boxes=finish_boxes(t.t.view(3, 40, 4), ref).view(3, 2, 20, 4))


# -- LayerNormFn
@case
class ln_plain:
    T = dict(x=A(2, 20, D), g=GAMMA(), be=B_())

    def gpu(t, Fn):
        return dict(y=Fn.layer_norm(t.x, t.g, t.be))

    def ref(t, r):
        return dict(y=ln(t.x, t.g, t.be))


@case
class ln_res_same:
    T = dict(x=A(2, 20, D), res=A(2, 20, D), g=GAMMA(), be=B_())

    def gpu(t, Fn):
        return dict(y=Fn.layer_norm(t.x, t.g, t.be, residual=t.res))

    def ref(t, r):
        return dict(y=ln(t.x + t.res, t.g, t.be))


@case
class ln_res_div:
    T = dict(x=A(3, 42, D), res=A(3, D), g=GAMMA(), be=B_())

    def gpu(t, Fn):
        return dict(y=Fn.layer_norm(t.x, t.g, t.be, residual=t.res, res_row_div=42))

    def ref(t, r):
        return dict(y=ln(t.x + t.res.repeat_interleave(42, 0).view(3, 42, D), t.g, t.be))


@case
class ln_stacked:
    T = dict(x0=A(2, 20, D), x1=A(2, 20, D), x2=A(2, 20, D), g=GAMMA(), be=B_())

    def gpu(t, Fn):
        return dict(y=Fn.layer_norm(torch.stack([t.x0, t.x1, t.x2]), t.g, t.be))

    def ref(t, r):
        return dict(y=ln(torch.stack([t.x0, t.x1, t.x2]), t.g, t.be))


# -- LinearAddNormFn(then=...)
class _Then:
    T = dict(a=A(2, 20, D), x=A(2, 20, D), w=W(), b=B_(), g=GAMMA(), be=B_(), tw=W(), tb=B_())

    @classmethod
    def gpu(cls, t, Fn):
        from future_od.switches import SW
        assert Fn.linear_add_norm_then_fits(t.a, t.w, t.tw)
        assert bool(SW.FOD_FUSED_LINEAR_PRE) == bool(cls.SWITCHES["FOD_FUSED_LINEAR_PRE"])
        y, nxt = Fn.linear_add_norm_then(t.a, t.x, t.w, t.b, t.g, t.be, t.tw, t.tb)
        if SW.FOD_FUSED_LINEAR_PRE:
            assert nxt.requires_grad
            return dict(y=y, nxt=nxt)
        assert not nxt.requires_grad
        yk, nxt = Fn.linear_keep(y, t.tw, t.tb, precomputed=nxt)
        return dict(y=yk, nxt=nxt)

    def ref(t, r):
        y = ln(t.x + lin(t.a, t.w, t.b), t.g, t.be)
        return dict(y=y * 1.0, nxt=lin(y, t.tw, t.tb))


@case
class lan_then_pre1(_Then):
    SWITCHES = dict(FOD_FUSED_LINEAR_PRE=1)


@case
class lan_then_pre0(_Then):
    SWITCHES = dict(FOD_FUSED_LINEAR_PRE=0)


# -- the packed input projections, each followed by the attention that sends dq | dk back
SCALE1 = 1.0 / math.sqrt(32)
SCALE2 = 1.0 / math.sqrt(64)


def _packed(t, r, xq, xk, xv):
    q = r(lin(xq, t.w[:D], t.b[:D]))
    k = r(lin(xk, t.w[D:2 * D], t.b[D:2 * D]))
    v = r(lin(xv, t.w[2 * D:], t.b[2 * D:]))
    return q, k, v


@case
class in_proj_attn:
    T = dict(xp=A(3, 42, D), src=A(3, 42, D), w=W(3 * D, D), b=B_(3 * D))
    S = dict(w=THIRDS, b=THIRDS)

    def gpu(t, Fn):
        q, k, v = Fn.in_proj(t.xp, t.src, t.w, t.b)
        assert Fn._column_siblings(q, k) is not None
        return dict(o=Fn.attention(q, k, v, SCALE1))

    def ref(t, r):
        q, k, v = _packed(t, r, t.xp, t.xp, t.src)
        return dict(o=r(attn(q, k, v, SCALE1)), _mass={("b", "k"): k})


class _InProjSelf:
    T = dict(src=A(3, 42, D), pos=A(42, D, grad=False), w=W(3 * D, D), b=B_(3 * D))
    S = dict(w=THIRDS, b=THIRDS)

    @classmethod
    def gpu(cls, t, Fn):
        res = Fn.in_proj_self(t.src, t.pos, t.w, t.b)
        assert res is not None
        keep, q, k, v = res
        o = Fn.attention(q, k, v, SCALE1)
        return dict(o=o, keep=keep) if cls.T["src"].grad else dict(o=o)

    @classmethod
    def ref(cls, t, r):
        pos = t.pos if t.pos.dim() == 3 else t.pos.repeat(3, 1).view(3, 42, D)
        xp = r(t.src + pos)
        q, k, v = _packed(t, r, xp, xp, t.src)
        o = r(attn(q, k, v, SCALE1))
        return dict(o=o, _mass={("b", "k"): k}, **(dict(keep=t.src * 1.0) if cls.T["src"].grad else {}))


@case
class in_proj_self_table(_InProjSelf):
    pass


@case
class in_proj_self_tensor(_InProjSelf):
    T = dict(_InProjSelf.T, pos=A(3, 42, D, grad=False))


@case
class in_proj_self_no_input_grad(_InProjSelf):
    T = dict(_InProjSelf.T, src=A(3, 42, D, grad=False))


@case
class in_proj_cross:
    T = dict(xq=A(3, 20, D), xk=A(3, 42, D, grad=False), xv=A(3, 42, D), w=W(3 * D, D), b=B_(3 * D))
    S = dict(w=THIRDS, b=THIRDS)

    def gpu(t, Fn):
        q, k, v = Fn.in_proj_cross(t.xq, t.xk, t.xv, t.w, t.b)
        return dict(o=Fn.attention(q, k, v, SCALE1))

    def ref(t, r):
        q, k, v = _packed(t, r, t.xq, t.xk, t.xv)
        return dict(o=r(attn(q, k, v, SCALE1)), _mass={("b", "k"): k})


@case
class attn_two_part_cross:
    T = dict(q1=A(2, 20, D), k1=A(2, 42, D), v=A(2, 42, D), q2=A(2, 20, D), k2=A(2, 42, D))

    def gpu(t, Fn):
        return dict(o=Fn.attention(t.q1, t.k1, t.v, SCALE2, t.q2, t.k2))

    def ref(t, r):
        return dict(o=attn(t.q1, t.k1, t.v, SCALE2, t.q2, t.k2))


# -- GroupLinearFn, WideLinearFn
def _lins(t, names):
    return [Lin(t["w" + n], t["b" + n]) for n in names]


def _grads_seen(**tensors):
    """{name: the gradient autograd hands to the producer of that tensor}, filled during the backward pass."""
    seen = {}
    for name, tensor in tensors.items():
        tensor.register_hook(lambda g, name=name: seen.__setitem__(name, g))
    return seen


def _params(names, n=D, k=D):
    out = {}
    for nm in names:
        out["w" + nm], out["b" + nm] = W(n, k), B_(n)
    return out


@case
class group_attn_self:
    """q, k, v of one grouped launch into self-attention: dq | dk | dv come back as consecutive blocks of one buffer."""
    T = dict(x=A(2, 20, D), **_params("qkv"))

    def gpu(t, Fn):
        q, k, v = Fn.group_linear(t.x, _lins(t, "qkv"))
        seen = _grads_seen(q=q, k=k, v=v)

        def after(t, Fn):
            if t.dtype == torch.bfloat16:       # (f32: three LinearFn nodes; the attention's buffer layout is the same)
                assert "GroupLinearFn" in q.grad_fn.name()
                assert Fn._as_segments([seen["q"], seen["k"], seen["v"]], 40, D) is not None     # taken as it is

        return dict(o=Fn.attention(q, k, v, SCALE1), _after=after)

    def ref(t, r):
        q, k, v = (r(lin(t.x, t["w" + n], t["b" + n])) for n in "qkv")
        return dict(o=r(attn(q, k, v, SCALE1)), _mass={("bk", ""): k})


class _GroupRes:
    """The self-attention's input side: the position tables of one grouped launch enter the first two results of another."""
    Bq = 2
    T = dict(x=A(2, 20, D), qpos=A(20, D), **_params("qkvrs"))

    @classmethod
    def gpu(cls, t, Fn):
        tabs = Fn.group_linear(t.qpos, _lins(t, "rs"))
        if t.dtype == torch.bfloat16:
            assert Fn._as_segments(tabs, 20, D) is not None
        q, k, v = Fn.group_linear(t.x, _lins(t, "qkv"), residual=tabs, res_row_mod=20)
        if t.dtype == torch.bfloat16:
            assert "GroupLinearFn" in q.grad_fn.name()          # the tables went into the launch, not into AddFn
        return dict(q=q, k=k, v=v)

    @classmethod
    def ref(cls, t, r):
        tq, tk = (r(lin(t.qpos, t["w" + n], t["b" + n])) for n in "rs")
        rep = lambda tab: tab.repeat(cls.Bq, 1).view(cls.Bq, 20, D)
        return dict(q=r(lin(t.x, t.wq, t.bq) + rep(tq)), k=r(lin(t.x, t.wk, t.bk) + rep(tk)), v=r(lin(t.x, t.wv, t.bv)))


@case
class group_res_rows_bm(_GroupRes):
    pass


@case
class group_res_rows_m(_GroupRes):
    Bq = 1
    T = dict(_GroupRes.T, x=A(1, 20, D))


@case
class group_unused_output:
    T = dict(x=A(2, 20, D), **_params("qkv"))

    def gpu(t, Fn):
        q, k, v = Fn.group_linear(t.x, _lins(t, "qkv"))
        seen = _grads_seen(q=q, k=k, v=v)

        def after(t, Fn):
            if t.dtype == torch.bfloat16:
                # one node: autograd has no gradient for the unused output (the hook sees None; backward gets None or the
                # zeros torch materialises for it), and the others are separate tensors, not blocks of one buffer --
                # _gather_segments copies them
                assert "GroupLinearFn" in q.grad_fn.name() and set(seen) == {"q", "k", "v"} and seen["k"] is None
                assert Fn._as_segments([seen["q"], seen["k"], seen["v"]], 40, D) is None
            else:
                assert set(seen) == {"q", "v"}      # three LinearFn nodes: the unused one never runs

        return dict(q=q, v=v, _after=after)

    def ref(t, r):
        return dict(q=lin(t.x, t.wq, t.bq), v=lin(t.x, t.wv, t.bv))


class _Wide:
    T = dict(x=A(2, 42, D), **_params("0123"))

    def gpu(t, Fn):
        return dict(y=Fn.wide_linear(t.x, _lins(t, "0123")), _after=lambda t, Fn: _queued(t, Fn, 1))

    def ref(t, r):
        return dict(y=torch.cat([lin(t.x, t["w" + n], t["b" + n]) for n in "0123"], -1))


@case
class wide_p4(_Wide):
    pass


@case
class wide_p4_table(_Wide):
    T = dict(_Wide.T, x=A(42, D, grad=False))


# -- Mlp2MulFn
def _mlp(t):
    return SimpleNamespace(layers=[Lin(t.w1, t.b1), Lin(t.w2, t.b2)], num_layers=2)


@case
class mlp2_shared3:
    """Three uses of one MLP on one table, as the decoder layers make them: the table's gradient is the sum over all three,
    delivered once, by the first call (the last to run in the backward pass)."""
    T = dict(x0=A(2, 20, D), x1=A(2, 20, D), x2=A(2, 20, D), table=A(20, D), **_params("12"))

    def gpu(t, Fn):
        class Acc(Fn.TableGradAcc):
            takes = 0

            def take(self):
                self.takes += 1
                return super().take()

        mlp, acc = _mlp(t), Acc()
        assert Fn.mlp2_mul_fits(t.x0, mlp, t.table)
        outs = {f"y{i}": Fn.mlp2_mul(t[f"x{i}"].view(40, D), mlp, t.table, acc=acc, hands_on=(i == 0)) for i in range(3)}

        def after(t, Fn):
            assert acc.buf is None and acc.takes == 1     # handed on, once: one gradient, not three for autograd to sum

        return dict(outs, _after=after)

    def ref(t, r):
        return {f"y{i}": lin(F.relu(lin(t[f"x{i}"].view(40, D), t.w1, t.b1)), t.w2, t.b2) * t.table.repeat(2, 1)
                for i in range(3)}


@case
class mlp2_single:
    T = dict(x=A(2, 20, D), table=A(20, D), **_params("12"))

    def gpu(t, Fn):
        assert Fn.mlp2_mul_fits(t.x, _mlp(t), t.table)
        return dict(y=Fn.mlp2_mul(t.x, _mlp(t), t.table))

    def ref(t, r):
        return dict(y=lin(F.relu(lin(t.x, t.w1, t.b1)), t.w2, t.b2) * t.table.repeat(2, 1).view(2, 20, D))


# -- ImuBranchFn
IMU_P, IMU_F, IMU_FF = 3, 5, 512


def _imu_params(use_mlp):
    out = {}
    for p in range(IMU_P):
        out.update({f"wv{p}": W(), f"bv{p}": B_(), f"wo{p}": W(), f"bo{p}": B_()})
        if use_mlp:
            out.update({f"g1{p}": GAMMA(), f"e1{p}": B_(), f"w0{p}": W(IMU_FF, D), f"b0{p}": B_(IMU_FF),
                        f"w3{p}": W(D, IMU_FF), f"b3{p}": B_(), f"g2{p}": GAMMA(), f"e2{p}": B_()})
    return out


def _imu_blocks(t, use_mlp):
    blocks = []
    for p in range(IMU_P):
        b = SimpleNamespace(value=Lin(t[f"wv{p}"], t[f"bv{p}"]), fun=SimpleNamespace(out_proj=Lin(t[f"wo{p}"], t[f"bo{p}"])),
                            use_mlp=use_mlp)
        if use_mlp:
            b.norm1, b.norm2 = Lin(t[f"g1{p}"], t[f"e1{p}"]), Lin(t[f"g2{p}"], t[f"e2{p}"])
            b.mlp = [Lin(t[f"w0{p}"], t[f"b0{p}"]), None, None, Lin(t[f"w3{p}"], t[f"b3{p}"])]
        blocks.append(b)
    return blocks


def _imu_ref(t, r, p, use_mlp):
    """out_proj(value(ego)) [-> norm1(o + o) -> o + MLP(o) -> norm2] of block p."""
    o = r(lin(r(lin(t.ego, t[f"wv{p}"], t[f"bv{p}"])), t[f"wo{p}"], t[f"bo{p}"]))
    if not use_mlp:
        return o
    n1 = r(ln(r(o + o), t[f"g1{p}"], t[f"e1{p}"]))
    h = r(F.relu(lin(n1, t[f"w0{p}"], t[f"b0{p}"])))
    y = r(lin(h, t[f"w3{p}"], t[f"b3{p}"]))
    return r(ln(r(n1 + y), t[f"g2{p}"], t[f"e2{p}"]))


class _Imu:
    use_mlp = False

    @classmethod
    def gpu(cls, t, Fn):
        blocks = _imu_blocks(t, cls.use_mlp)
        assert Fn.imu_branch_fits(t.ego, blocks)
        outs = Fn.imu_branch(t.ego, blocks)
        return {f"e{p}": outs[p] for p in range(IMU_P)}

    @classmethod
    def ref(cls, t, r):
        return {f"e{p}": _imu_ref(t, r, p, cls.use_mlp) for p in range(IMU_P)}


@case
class imu_plain(_Imu):
    T = dict(ego=A(IMU_F, D, s=0.7), **_imu_params(False))


@case
class imu_mlp(_Imu):
    use_mlp = True
    T = dict(ego=A(IMU_F, D, s=0.7), **_imu_params(True))


@case
class imu_queue_norms:
    """The encoder's IMU rows: the blocks of P layers at once, each layer's norm adds its row to the frame's N tokens and
    leaves the sum of its gradient over those tokens to the queue, which fills all P slots in one launch when
    ImuBranchFn.backward is reached."""
    N = 42
    T = dict(ego=A(IMU_F, D, s=0.7), **_imu_params(False),
             **{f"x{p}": A(IMU_F, 42, D) for p in range(IMU_P)},
             **{f"g{p}": GAMMA() for p in range(IMU_P)}, **{f"be{p}": B_() for p in range(IMU_P)})

    def gpu(t, Fn):
        queue = Fn.ResGradQueue(IMU_P)
        es = Fn.imu_branch(t.ego, _imu_blocks(t, False), queue=queue)
        outs = {f"y{p}": Fn.layer_norm(t[f"x{p}"], t[f"g{p}"], t[f"be{p}"], residual=es[p], res_row_div=42,
                                       res_queue=queue, res_slot=p) for p in range(IMU_P)}

        def after(t, Fn):
            assert queue.buf is not None and tuple(queue.buf.shape) == (IMU_P, IMU_F, D) and not queue.jobs

        return dict(outs, _after=after)

    def ref(t, r):
        outs = {}
        for p in range(IMU_P):
            e = _imu_ref(t, r, p, False)
            s = r(t[f"x{p}"] + e.repeat_interleave(42, 0).view(IMU_F, 42, D))
            outs[f"y{p}"] = r(ln(s, t[f"g{p}"], t[f"be{p}"]))
        return outs


# -- the memory side of the decoder
MEM_L, MEM_K, MEM_B, MEM_M = 2, 2, 2, 20
_LJ = [(l, j) for l in range(MEM_L) for j in range(MEM_K)]             # forward order: layer-major


class _Memory:
    N, per_batch = 42, False

    @classmethod
    def tensors(cls):
        out = {f"mem{j}": A(MEM_B, cls.N, D) for j in range(MEM_K)}
        out["pos"] = A(MEM_B, cls.N, D) if cls.per_batch else A(cls.N, D)
        for l, j in _LJ:
            out.update({f"q1_{l}{j}": A(MEM_B, MEM_M, D), f"q2_{l}{j}": A(MEM_B, MEM_M, D)})
            out.update(_params([f"v{l}{j}", f"c{l}{j}", f"p{l}{j}"]))
        return out

    S = dict(big0=cols(2 * MEM_L, D, "slot"), big1=cols(2 * MEM_L, D, "slot"), ks_all=cols(MEM_L * MEM_K, D, "slot"))

    @classmethod
    def gpu(cls, t, Fn):
        big = [Fn.wide_linear(t[f"mem{j}"], [m for l in range(MEM_L) for m in _lins(t, [f"v{l}{j}", f"c{l}{j}"])])
               for j in range(MEM_K)]
        ks_all = Fn.wide_linear(t.pos, _lins(t, [f"p{l}{j}" for l, j in _LJ]))
        assert ks_all.dim() == (3 if cls.per_batch else 2)
        side = Fn.MemorySide(big, ks_all, MEM_L, MEM_K, D)
        outs = {f"o{l}{j}": Fn.hoisted_cross_attention(t[f"q1_{l}{j}"], t[f"q2_{l}{j}"], side, l, j, SCALE2) for l, j in _LJ}
        # a second consumer of every hoisted buffer, with a zero gradient that reaches the buffer's producer FIRST: autograd
        # then ADDS what a cross-attention call hands on, at that moment -- a buffer handed on before its last slot is
        # filled (by any call but layer 0's) is summed as it is then, and the slots written later are lost
        outs.update(z0=big[0] * 0.0, z1=big[1] * 0.0, zk=ks_all * 0.0)

        def after(t, Fn):
            queued = getattr(side, "dkv_queue", None) is not None
            assert queued == (cls.N >= 256 and t.dtype == torch.bfloat16), queued
            assert not queued or not side.dkv_queue.jobs
            assert all(d is not None for d in side.dbig) and side.dks is not None and side.dks.dim() == 3

        return dict(outs, _keep=dict(big0=big[0], big1=big[1], ks_all=ks_all), _after=after)

    @classmethod
    def ref(cls, t, r):
        big = []
        for j in range(MEM_K):
            big.append(torch.cat([lin(t[f"mem{j}"], t[f"w{n}{l}{j}"], t[f"b{n}{l}{j}"]) for l in range(MEM_L) for n in "vc"], -1))
        ks_all = torch.cat([lin(t.pos, t[f"wp{l}{j}"], t[f"bp{l}{j}"]) for l, j in _LJ], -1)
        bigr, ksr = [r(b) for b in big], r(ks_all)
        outs, mass = {}, {}
        for l, j in _LJ:
            v = bigr[j][..., (2 * l) * D:(2 * l + 1) * D]
            kc = bigr[j][..., (2 * l + 1) * D:(2 * l + 2) * D]
            qi = l * MEM_K + j
            ks = ksr[..., qi * D:(qi + 1) * D]
            if ks.dim() == 2:                # shared by the batch: the per-batch gradients are stored, then summed
                ks = r(ks.unsqueeze(0).repeat(MEM_B, 1, 1))
            outs[f"o{l}{j}"] = r(attn(t[f"q1_{l}{j}"], kc, v, SCALE2, t[f"q2_{l}{j}"], ks))
            mass[(f"bc{l}{j}", "")], mass[(f"bp{l}{j}", "")] = kc, ks
        outs.update(z0=big[0] * 0.0, z1=big[1] * 0.0, zk=ks_all * 0.0)
        return dict(outs, _keep=dict(big0=big[0], big1=big[1], ks_all=ks_all), _mass=mass)


@case
class memory_n42_shared(_Memory):
    pass


@case
class memory_n42_per_batch(_Memory):
    per_batch = True


@case
class memory_n272_shared(_Memory):
    N = 272


@case
class memory_n272_per_batch(_Memory):
    N, per_batch = 272, True


for _c in (memory_n42_shared, memory_n42_per_batch, memory_n272_shared, memory_n272_per_batch):
    _c.T = _c.tensors()


# ------------------------------------------------------------------------------------------------ Case.measured
def measure(name):
    """{slice: error} of the rounded float64 reference of a case against the plain one (bf16)."""
    case = CASES[name]
    plain, rounded = run_ref(case, "bf16"), run_ref(case, "bf16", rounded=True)
    slices = getattr(case, "S", {})
    figures = []
    for kind, a, b in zip(("out", "d", "d"), rounded[:3], plain[:3]):
        for n, w in b.items():
            if w is not None:
                _compare(kind, n, a[n], w, slices.get(n, WHOLE), lambda what: float("inf"), [], figures, plain[3])
    return dict(figures)


def measured_as_recorded(name):
    """What Case.measured of `name` would be today, in the form the table records it: one figure (the largest over the
    slices), or, for a per-slice record, the listed slices and "" for the largest of the others."""
    figures, recorded = measure(name), NC.CASES[name].measured
    if not isinstance(recorded, dict):
        return max(figures.values())
    out = {k: figures[k] for k in recorded if k}
    out[""] = max(v for k, v in figures.items() if k not in recorded)
    return out


if __name__ == "__main__":
    for _name in ([a for a in sys.argv[1:] if a != "-v"] or [n for n, c in NC.CASES.items() if c.measured is not None]):
        _figures = measure(_name)
        _where = max(_figures, key=_figures.get)
        print(f"{_name}: measured {_figures[_where]:.2e} at {_where}  (table: {NC.CASES[_name].measured})")
        if "-v" in sys.argv:
            print("  " + ", ".join(f"{n} {e:.2e}" for n, e in _figures.items()))
