"""Autograd glue: each Function's forward and backward are calls into libfod_hip.so.

Parameters are fp32; kernels consume prepared copies of them (native/prepared.py).  Activations and their gradients are
in the compute dtype (torch.float32 = parity mode, torch.bfloat16 = performance mode); parameter gradients are fp32
slices of the zero arena (native/arena.py), the short and the long ones filled by the queue of native/wgrad.py.
"""
import torch
from torch.autograd import Function

from . import lib as L
from . import ops
# re-exported for callers; a registry that may be REBOUND (a test swaps prepared.PREP) is read through its own module
from .arena import ARENA, _ZeroArena, zeros_f32
from .prepared import (CAT, PREP, STACK, _Job, _Prepared, _VEC, _pad_to, _wkey, prep_conv, prep_linear,
                       prep_stem)
from .wgrad import WGRADS, _WgradQueue
from ..switches import SW

# Data-parallel runs: the object that averages finished arena regions across ranks (parallel.GradientReducer),
# installed by FodDataParallel.forward for the coming backward pass; None otherwise.
GRAD_SYNC = None


# Deterministic mode (one switch for the whole kernel layer; see native/ops.py): Fn.set_deterministic(True), or
# FOD_DETERMINISTIC=1 in the environment, or build_model(args) with args.deterministic.  Default: off.
set_deterministic = ops.set_deterministic
is_deterministic = ops.is_deterministic


def set_grad_sync(reducer):
    global GRAD_SYNC
    GRAD_SYNC = reducer


class BackboneCut:
    """Cuts the autograd graph at the backbone's output so that a backward pass can run in TWO pieces: `loss.backward()`
    stops at the returned leaf (every transformer gradient + d loss / d features), `finish()` then runs the backbone's
    backward from it.  A data-parallel captured step (future_od/graph.py) puts the two pieces into separate graphs and
    averages the transformer gradients across ranks WHILE the backbone piece runs."""

    def __init__(self):
        self.pairs = []

    def cut(self, feat):
        leaf = feat.detach().requires_grad_(True)
        self.pairs.append((feat, leaf))
        return leaf

    def finish(self):
        pairs, self.pairs = self.pairs, []
        if pairs:
            torch.autograd.backward([f for f, _ in pairs], [l.grad for _, l in pairs])


BACKBONE_CUT = None


def cast(t, dtype, pad_cols=None):
    """[rows, cols] tensor -> dtype, optionally zero-padding the last dim."""
    cols = t.shape[-1]
    rows = t.numel() // cols
    t = t.contiguous()
    pc = cols if pad_cols is None else pad_cols
    return ops.permute3_cast(t, dtype, (1, rows, pc), (0, cols, 1), valid2=cols).view(*t.shape[:-1], pc)


def _grad_rows(dy, cols, dtype):
    """An incoming gradient as [rows, cols] in the compute dtype."""
    g = dy.contiguous().view(-1, cols)
    return g if g.dtype == dtype else cast(g, dtype)


def _param_grads(weight, bias, g, x, need_w, need_b, shared):
    """(dw, db) of y = x W^T + b from g = dy [rows, N] and x [rows, K]: the weight gradient through the queue, the bias
    gradient from the same pass.  `shared`: the layer may be used several times in a backward pass; a further use is
    summed inside the first use's job (WGRADS.chain) and gets (None, None)."""
    want_db = bias is not None and need_b
    if shared and need_w and WGRADS.chain(weight, want_db, g, x):
        return None, None
    db = zeros_f32((g.shape[-1],), x.device) if want_db else None
    dw = None
    if need_w:
        dw = zeros_f32((g.shape[-1], x.shape[-1]), x.device)
        WGRADS.tn(WGRADS.site((weight, bias)), g, x, dw, db, owner=weight if shared else None)
    elif want_db:
        ops.colsum_acc(g, db)
    return dw, db


# ------------------------------------------------------------------------------------------------
class LinearFn(Function):
    """y = act(x W^T + b) (+ residual)."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu, out_f32):
        dtype = x.dtype
        w = prep_linear(weight, dtype, False)
        N = weight.shape[0]
        y = ops.gemm_nt(x, w[:N] if w.shape[0] != N else w, shift=bias, relu=relu, out_f32=out_f32)
        y = y.view(*x.shape[:-1], N)
        ctx.relu, ctx.out_f32 = relu, out_f32
        ctx.weight, ctx.bias = weight, bias
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y = ctx.saved_tensors
        weight = ctx.weight
        dtype = x.dtype
        N, K = weight.shape
        v = _VEC[dtype]
        Np = _pad_to(N, v)
        dy = dy.contiguous()
        if dy.dtype != dtype or Np != N:
            g = cast(dy.view(-1, N), dtype, pad_cols=Np)
        else:
            g = dy.view(-1, N)
        if ctx.relu:
            assert Np == N
            g = ops.eltwise(L.EW_RELU_MASK, g, y.view(-1, N))
        dx = None
        if ctx.needs_input_grad[0]:
            dx = ops.gemm_nt(g, prep_linear(weight, dtype, True)).view(x.shape)
        dw, db = _param_grads(weight, ctx.bias, g, x.view(-1, K), ctx.needs_input_grad[1], ctx.needs_input_grad[2], True)
        if Np != N:                                  # the gradients of the padded rows stay behind
            dw, db = (None if dw is None else dw[:N]), (None if db is None else db[:N])
        return dx, dw, db, None, None


def linear(x, weight, bias=None, relu=False, out_f32=False):
    return LinearFn.apply(x.contiguous(), weight, bias, relu, out_f32)


class LinearKeepFn(Function):
    """(x, act(x W^T + b)): the projection of a tensor that is ALSO the residual of the sub-layer it opens.  As two
    consumers of x, autograd would sum their gradients with a kernel of its own (a 5 us graph node per sub-layer, ~45 per
    step); here the residual path's gradient enters the projection's input-gradient GEMM as its epilogue operand."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu, grad_masked=False, precomputed=None):
        """`grad_masked` (with relu): the consumer of y applies the (y > 0) mask to the gradient it sends back
        (LinearAddNormFn(a_relu=True)); this node then skips its own masking pass.  `precomputed`: act(x W^T + b) as the
        launch that produced x already computed it (LinearAddNormFn(then=...)): no launch here, the same backward."""
        dtype = x.dtype
        N = weight.shape[0]
        if precomputed is not None:
            y = precomputed.view(*x.shape[:-1], N)
        else:
            w = prep_linear(weight, dtype, False)
            y = ops.gemm_nt(x, w[:N] if w.shape[0] != N else w, shift=bias, relu=relu).view(*x.shape[:-1], N)
        ctx.relu, ctx.weight, ctx.bias, ctx.has_bias = relu, weight, bias, bias is not None
        ctx.mask_here = relu and not grad_masked
        ctx.save_for_backward(x, y if ctx.mask_here else None)
        return x.view_as(x), y

    @staticmethod
    def backward(ctx, dkeep, dy):
        x, y = ctx.saved_tensors
        weight = ctx.weight
        dtype = x.dtype
        N, K = weight.shape
        assert N % _VEC[dtype] == 0
        g = _grad_rows(dy, N, dtype)
        if ctx.mask_here:
            g = ops.eltwise(L.EW_RELU_MASK, g, y.view(-1, N))
        dx = None
        if ctx.needs_input_grad[0]:
            res = None if dkeep is None else _grad_rows(dkeep, K, dtype)
            dx = ops.gemm_nt(g, prep_linear(weight, dtype, True), residual=res).view(x.shape)
        dw, db = _param_grads(weight, ctx.bias, g, x.view(-1, K), ctx.needs_input_grad[1], ctx.needs_input_grad[2], False)
        return dx, dw, db, None, None, None


def linear_keep(x, weight, bias=None, relu=False, grad_masked=False, precomputed=None):
    """-> (x for the residual path, act(x W^T + b)); see LinearKeepFn.  Falls back to two consumers when the output
    width does not fit the vector epilogue (that path masks its own gradient: a second mask upstream is harmless)."""
    if weight.shape[0] % _VEC[x.dtype] != 0 or not SW.FOD_LINEAR_KEEP:
        assert precomputed is None
        return x, linear(x, weight, bias, relu=relu)
    return LinearKeepFn.apply(x.contiguous(), weight, bias, relu, grad_masked, precomputed)


class AddFn(Function):
    """a + b[row(m)], b broadcast over row groups (div) or periodically (mod)."""

    @staticmethod
    def forward(ctx, a, b, b_row_div, b_row_mod):
        ctx.cfg = (b_row_div, b_row_mod, b.shape, a.shape)
        return ops.eltwise(L.EW_ADD, a, b, b_row_div=b_row_div, b_row_mod=b_row_mod)

    @staticmethod
    def backward(ctx, g):
        div, mod, bshape, ashape = ctx.cfg
        g = g.contiguous()
        db = None
        if ctx.needs_input_grad[1]:
            cols = ashape[-1]
            rows = g.numel() // cols
            if not div and not mod:
                db = g.view(bshape)
            elif mod and not div:
                db = _sum_periodic(g.view(rows, cols), mod).view(bshape)
            else:
                assert not mod
                out = zeros_f32((rows // div, cols), g.device)
                ops.colsum_acc(g.view(rows, cols), out, group_rows=div)
                db = cast(out, g.dtype).view(bshape)
        return (g.view(ashape) if ctx.needs_input_grad[0] else None), db, None, None


def add(a, b, b_row_div=0, b_row_mod=0):
    return AddFn.apply(a.contiguous(), b.contiguous(), b_row_div, b_row_mod)


class MulFn(Function):
    """a * b[m % b_row_mod] (b broadcast periodically over the rows of a when b_row_mod > 0)."""

    @staticmethod
    def forward(ctx, a, b, b_row_mod):
        ctx.save_for_backward(a, b)
        ctx.mod = b_row_mod
        return ops.eltwise(L.EW_MUL, a, b, b_row_mod=b_row_mod)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = g.contiguous()
        da = ops.eltwise(L.EW_MUL, g, b, b_row_mod=ctx.mod)
        db = ops.eltwise(L.EW_MUL, g, a)
        if ctx.mod:
            db = _sum_periodic(db, ctx.mod).view(b.shape)
        return da, db, None


class TableGradAcc:
    """One f32 accumulation buffer for the gradient of a table that several Mlp2MulFn nodes multiply by (the decoder
    layers' query_scale(x) * sine embedding): every node's backward launch adds into it (atomics on the default path, row-ordered sums in deterministic mode); the node that runs
    LAST in the backward pass (the first in the forward pass: later layers depend on its output) hands the total on --
    one gradient instead of one per layer that autograd would sum with kernels of its own."""

    def __init__(self):
        self.buf = None

    def get(self, shape, device):
        if self.buf is None:
            self.buf = zeros_f32(shape, device)
        return self.buf

    def take(self):
        buf, self.buf = self.buf, None
        return buf


class Mlp2MulFn(Function):
    """((relu(x W1^T + b1)) W2^T + b2) * table[m % rows(table)] as ONE launch forward and ONE backward
    (fod_mlp2_mul_fwd / _bwd, csrc/linear_norm.hip): reference transformer.py:384-386, once per decoder layer.  As separate
    nodes that was 2 GEMMs + a multiply forward and 2 GEMMs + a ReLU gate + 2 multiplies + a sum over the batch backward."""

    @staticmethod
    def forward(ctx, x, table, w1, b1, w2, b2, acc, hands_on):
        D = x.shape[-1]
        x2 = x.view(-1, D)
        out, h, q = ops.mlp2_mul_fwd(x2, prep_linear(w1, x.dtype, False), b1, prep_linear(w2, x.dtype, False), b2, table)
        ctx.save_for_backward(x2, h, q, table)
        ctx.params, ctx.acc, ctx.hands_on, ctx.x_shape = (w1, b1, w2, b2), acc, hands_on, x.shape
        return out.view(x.shape)

    @staticmethod
    def backward(ctx, g):
        x2, h, q, table = ctx.saved_tensors
        w1, b1, w2, b2 = ctx.params
        D = x2.shape[-1]
        g = _grad_rows(g, D, x2.dtype)
        acc = ctx.acc if ctx.acc is not None else TableGradAcc()
        buf = acc.get(tuple(table.shape), x2.device)
        ds, dh, dx = ops.mlp2_mul_bwd(g, table, q, h, prep_linear(w2, x2.dtype, True), prep_linear(w1, x2.dtype, True), buf)
        dw2, db2 = _param_grads(w2, b2, ds, h, ctx.needs_input_grad[4], ctx.needs_input_grad[5], True)
        dw1, db1 = _param_grads(w1, b1, dh, x2, ctx.needs_input_grad[2], ctx.needs_input_grad[3], True)
        dtable = None
        if ctx.needs_input_grad[1] and (ctx.acc is None or ctx.hands_on):
            dtable = cast(acc.take(), table.dtype).view(table.shape)
        # (x's own shape: the decoder hands in [B * M, D], but the wrapper takes any [..., D])
        return (dx.view(ctx.x_shape) if ctx.needs_input_grad[0] else None), dtable, dw1, db1, dw2, db2, None, None


def mlp2_mul_fits(x, mlp, table):
    """Whether Mlp2MulFn applies: bf16, a two-layer 256 -> 256 -> 256 MLP with biases, a [rows, 256] table dividing x's rows."""
    if not SW.FOD_FUSED_MLP2 or x.dtype != torch.bfloat16 or getattr(mlp, "num_layers", 0) != 2:
        return False
    l0, l1 = mlp.layers
    D = x.shape[-1]
    return (D == 256 and tuple(l0.weight.shape) == (D, D) and tuple(l1.weight.shape) == (D, D) and l0.bias is not None
            and l1.bias is not None and table.dtype == x.dtype and table.dim() == 2 and table.shape[1] == D
            and (x.numel() // D) % table.shape[0] == 0)


def mlp2_mul(x, mlp, table, acc=None, hands_on=True):
    """mlp(x) * table[m % rows(table)] (see Mlp2MulFn).  `acc` (TableGradAcc) shared by several calls on one table: only the
    call with hands_on=True -- the FIRST of them in the forward pass -- returns the table's (total) gradient."""
    l0, l1 = mlp.layers
    return Mlp2MulFn.apply(x.contiguous(), table.contiguous(), l0.weight, l0.bias, l1.weight, l1.bias, acc, hands_on)


def _sum_periodic(g, mod):
    """[rows, cols] -> [mod, cols]: sum of the rows congruent modulo `mod` (rows/mod is tiny)."""
    parts = g.view(-1, mod, g.shape[-1])
    return _sum_leading(parts, parts.shape[0])


def mul(a, b, b_row_mod=0):
    return MulFn.apply(a.contiguous(), b.contiguous(), b_row_mod)


class ExpandRowsFn(Function):
    """[rows, cols] -> [reps*rows, cols] (periodic copy); backward sums the copies."""

    @staticmethod
    def forward(ctx, x, reps):
        rows, cols = x.shape
        ctx.rows = rows
        out = torch.empty((reps * rows, cols), dtype=x.dtype, device=x.device)
        return ops.eltwise(L.EW_COPY_B, out, x, b_row_mod=rows, out=out)

    @staticmethod
    def backward(ctx, g):
        return _sum_periodic(g.contiguous(), ctx.rows), None


def expand_rows(x, reps):
    return ExpandRowsFn.apply(x.contiguous(), reps)


class ResGradQueue:
    """The gradients of P broadcast residual rows ([groups, D] each: the per-frame IMU rows that P encoder layers add to
    their tokens) as slots of ONE [P, groups, D] buffer, filled by ONE launch (fod_colsum_groups_multi) when their reader
    -- ImuBranchFn.backward -- is reached: a LayerNormFn whose residual is such a row hands its gradient's tokens over
    and returns the (still unfilled) slot."""

    def __init__(self, P):
        self.P, self.buf, self.jobs, self.geom = P, None, [], None

    def push(self, slot, g, groups, group_rows, D):
        if self.buf is None:
            self.buf = torch.empty((self.P, groups, D), dtype=g.dtype, device=g.device)
        geom = (groups, group_rows, D)
        assert self.geom in (None, geom) and tuple(self.buf.shape[1:]) == (groups, D)
        self.geom = geom
        self.jobs.append((g, self.buf[slot]))
        return self.buf[slot]

    def flush(self):
        if self.jobs:
            jobs, self.jobs = self.jobs, []
            for i in range(0, len(jobs), 16):
                ops.colsum_groups_multi(jobs[i:i + 16], *self.geom)


class LayerNormFn(Function):
    """LayerNorm(x + residual[row(m)]) over the last dim."""

    @staticmethod
    def forward(ctx, x, residual, gamma, beta, res_row_div, res_queue=None, res_slot=0):
        y, s, mean, rstd = ops.layernorm_fwd(x, gamma, beta, residual=residual, res_row_div=res_row_div)
        ctx.save_for_backward(s, mean, rstd, gamma)
        ctx.res_row_div = res_row_div
        ctx.res_shape = None if residual is None else residual.shape
        ctx.res_queue, ctx.res_slot = res_queue, res_slot
        return y

    @staticmethod
    def backward(ctx, dy):
        s, mean, rstd, gamma = ctx.saved_tensors
        D = gamma.numel()
        dg = zeros_f32((D,), dy.device)
        db = zeros_f32((D,), dy.device)
        dx = ops.layernorm_bwd(dy.contiguous(), s, mean, rstd, gamma, dg, db)
        dres = None
        if ctx.res_shape is not None and ctx.needs_input_grad[1]:
            rows = dx.numel() // D
            if (ctx.res_row_div and ctx.res_queue is not None and dx.dtype == torch.bfloat16 and D <= 256 and D % 4 == 0
                    and rows % ctx.res_row_div == 0):
                # the sum over each frame's tokens waits for the other layers' (ResGradQueue): the slot is filled later
                dres = ctx.res_queue.push(ctx.res_slot, dx.view(rows, D), rows // ctx.res_row_div, ctx.res_row_div,
                                          D).view(ctx.res_shape)
            elif ctx.res_row_div:
                out = zeros_f32((rows // ctx.res_row_div, D), dy.device)
                ops.colsum_acc(dx.view(rows, D), out, group_rows=ctx.res_row_div)
                dres = cast(out, dx.dtype).view(ctx.res_shape)
            else:
                dres = dx.view(ctx.res_shape)
        return dx, dres, dg, db, None, None, None


def layer_norm(x, gamma, beta, residual=None, res_row_div=0, res_queue=None, res_slot=0):
    """res_queue / res_slot (with res_row_div): the residual's gradient is summed later, with the other slots of the queue."""
    return LayerNormFn.apply(x.contiguous(), None if residual is None else residual.contiguous(), gamma, beta,
                             res_row_div, res_queue, res_slot)


# FOD_FUSED_LINEAR_NORM_ROWS: rows up to which the fused projection + norm launches (fod_linear_add_norm_fwd / _bwd, with
# their then_* and pre_* parts) are used.  The kernels walk 16-row tiles with the weights stationary, so they take any
# row count, but at the encoder's 14 500 rows they do not pay (one wave per SIMD, every tile's loads queue behind the
# previous tile's stores): forward 19.5 us against 21.3 for GEMM + norm, backward 26.3 against 20.9, whole step +0.1 ms
# (profiles/r03l_fused_linear_norm.txt)


class LinearAddNormFn(Function):
    """y = LayerNorm(x + (a W^T + b)): a sub-layer's output projection, the residual add and the post-norm as ONE
    autograd node -- the same two kernels forward and four backward as LinearFn + LayerNormFn, but one Function
    application instead of two per site (~55 sites per step; the launching thread is the bottleneck on slow hosts).
    Used where no dropout sits between the projection and the add (eval mode or p = 0)."""

    @staticmethod
    def forward(ctx, a, x, weight, bias, gamma, beta, a_relu=False, then_weight=None, then_bias=None):
        """`a_relu`: `a` is the output of a ReLU whose producer leaves the masking of its incoming gradient to THIS
        node (LinearKeepFn(grad_masked=True)): the (a > 0) mask is applied in the epilogue of the GEMM that forms da --
        one pass over a [rows, 2048] gradient less per feed-forward block."""
        N = weight.shape[0]
        w = prep_linear(weight, a.dtype, False)
        assert w.shape[0] == N, "linear_add_norm: out_features must be a multiple of the vector width"
        rows = a.numel() // a.shape[-1]
        if (SW.FOD_FUSED_LINEAR_NORM and a.dtype == torch.bfloat16 and N == 256 and weight.shape[1] == 256 and w.shape[1] == 256
                and rows <= SW.FOD_FUSED_LINEAR_NORM_ROWS):
            # the decoder's query side: projection + residual add + norm as ONE launch (csrc/linear_norm.hip)
            if then_weight is not None:
                # ... and the next block's 256 -> 256 projection of y from the same launch: a CONSTANT second output
                # that LinearKeepFn(precomputed=...) adopts as its result (its backward is the usual one)
                y, s, mean, rstd, nxt = ops.linear_add_norm_fwd(a, w, bias, x, gamma, beta,
                                                                then_w=prep_linear(then_weight, a.dtype, False),
                                                                then_bias=then_bias)
            else:
                y, s, mean, rstd = ops.linear_add_norm_fwd(a, w, bias, x, gamma, beta)
        else:
            assert then_weight is None, "linear_add_norm(then=...) outside the fused launch's domain (the caller checks)"
            o = ops.gemm_nt(a, w, shift=bias).view(x.shape)
            y, s, mean, rstd = ops.layernorm_fwd(x, gamma, beta, residual=o)
        ctx.then = None
        ctx.weight, ctx.bias, ctx.has_bias, ctx.a_relu = weight, bias, bias is not None, bool(a_relu)
        if then_weight is not None and SW.FOD_FUSED_LINEAR_PRE:
            # the second result is differentiable: its gradient comes back to THIS node (backward's pre form)
            ctx.then = (then_weight, then_bias)
            ctx.save_for_backward(a, s, mean, rstd, gamma, y)
            return y, nxt
        ctx.save_for_backward(a, s, mean, rstd, gamma)
        if then_weight is not None:
            ctx.mark_non_differentiable(nxt)
            return y, nxt
        return y

    @staticmethod
    def backward(ctx, dy, dnxt=None):
        a, s, mean, rstd, gamma = ctx.saved_tensors[:5]
        weight = ctx.weight
        N, K = weight.shape
        dev = s.device
        dg, dbeta = zeros_f32((N,), dev), zeros_f32((N,), dev)
        da = None
        rows = s.numel() // N
        dw2 = db2 = pre_g = pre_wt = None
        if ctx.then is not None and dnxt is not None:
            # the THEN projection's own gradients: its weight / bias through the queue (dq^T y), its input gradient
            # dq . then_w joins dy inside the fused launch below (or through a GEMM epilogue on the fallback path)
            then_w, then_b = ctx.then
            y = ctx.saved_tensors[5]
            pre_g = _grad_rows(dnxt, N, a.dtype)
            pre_wt = prep_linear(then_w, a.dtype, True)
            dw2, db2 = _param_grads(then_w, then_b, pre_g, y.view(-1, N), ctx.needs_input_grad[7], ctx.needs_input_grad[8],
                                    False)
        if dy is not None:
            dy = dy.contiguous()
        if (SW.FOD_FUSED_LINEAR_NORM and s.dtype == torch.bfloat16 and N == 256 and K == 256 and rows <= SW.FOD_FUSED_LINEAR_NORM_ROWS
                and ctx.needs_input_grad[0] and not ctx.a_relu):
            # the decoder's query side: layer-norm gradient and the projection's input gradient as ONE launch
            wt = prep_linear(weight, a.dtype, True)
            assert tuple(wt.shape) == (K, N)
            dsum, da = ops.linear_add_norm_bwd(dy, s, mean, rstd, gamma, wt, dg, dbeta, pre_g=pre_g, pre_w_t=pre_wt)
            dsum, da = dsum.view(s.shape), da.view(a.shape)
            g = dsum.view(-1, N)
        else:
            if pre_g is not None:
                dy = ops.gemm_nt(pre_g, pre_wt, residual=None if dy is None else dy.view(-1, N)).view(s.shape)
            dsum = ops.layernorm_bwd(dy.contiguous(), s, mean, rstd, gamma, dg, dbeta)     # d(x + o): feeds both branches
            g = dsum.view(-1, N)
            if ctx.needs_input_grad[0]:
                da = ops.gemm_nt(g, prep_linear(weight, a.dtype, True),
                                 relu_mask=a.view(-1, K) if ctx.a_relu else None).view(a.shape)
        dw, db = _param_grads(weight, ctx.bias, g, a.view(-1, K), ctx.needs_input_grad[2], ctx.needs_input_grad[3], False)
        return da, (dsum if ctx.needs_input_grad[1] else None), dw, db, dg, dbeta, None, dw2, db2


def linear_add_norm(a, x, weight, bias, gamma, beta, a_relu=False):
    return LinearAddNormFn.apply(a.contiguous(), x.contiguous(), weight, bias, gamma, beta, a_relu, None, None)


def linear_add_norm_then_fits(a, weight, then_weight):
    """Whether linear_add_norm_then may be used: the fused launch's domain (bf16, 256-wide projections, few rows)."""
    rows = a.numel() // a.shape[-1]
    return (SW.FOD_FUSED_LINEAR_NORM and SW.FOD_FUSED_LINEAR_THEN and a.dtype == torch.bfloat16 and tuple(weight.shape) == (256, 256)
            and tuple(then_weight.shape) == (256, 256) and rows <= SW.FOD_FUSED_LINEAR_NORM_ROWS and SW.FOD_LINEAR_KEEP)


def linear_add_norm_then(a, x, weight, bias, gamma, beta, then_weight, then_bias):
    """(y, y then_weight^T + then_bias) with y = LayerNorm(x + a W^T + b): ONE launch.  With FOD_FUSED_LINEAR_PRE the second
    result is a differentiable output of this node (use it as it is: its gradient returns here and the backward launch
    forms dq . then_weight itself); without, it is a constant for autograd -- hand it to
    linear_keep(y, then_weight, then_bias, precomputed=...), whose backward needs nothing else."""
    return LinearAddNormFn.apply(a.contiguous(), x.contiguous(), weight, bias, gamma, beta, False, then_weight, then_bias)


# ------------------------------------------------------------------------------------------------
class ConvFn(Function):
    """y = act(conv2d(x, W) + b) on NHWC activations: a stand-alone trainable convolution (the backbone has its own
    whole-network node, native/backbone.py).  W is an OIHW parameter (any strides with a dense tap plane), stride 1,
    padding k // 2.  Backward: ReLU mask, input gradient, weight gradient (f32 atomics on the default path, fixed-order partial sums in deterministic mode, into a [Cout][kh][kw][Cin]
    buffer returned as an OIHW view), bias gradient."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu):
        co, ci, kh, kw = weight.shape
        geom = ops.conv_geom(x.shape, co, kh, 1, kh // 2)
        y = ops.conv2d_fwd(x, prep_conv(weight, x.dtype, None, False), geom, shift=bias, relu=relu)
        ctx.save_for_backward(x, y if relu else None)
        ctx.weight, ctx.geom, ctx.relu, ctx.has_bias = weight, geom, relu, bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y = ctx.saved_tensors
        weight, geom = ctx.weight, ctx.geom
        co, ci, kh, kw = weight.shape
        g = dy.contiguous()
        if ctx.relu:
            g = ops.eltwise(L.EW_RELU_MASK, g.view(-1, co), y.view(-1, co)).view(dy.shape)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = ops.conv2d_dgrad(g, prep_conv(weight, x.dtype, None, True), geom)
        if ctx.needs_input_grad[1]:
            buf = zeros_f32((co, kh, kw, ci), x.device)
            ops.conv2d_wgrad_acc(g, x, buf, geom, zeroed=True)
            dw = buf.view(co, ci, 1, 1) if kh == 1 and kw == 1 else buf.permute(0, 3, 1, 2)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = zeros_f32((co,), x.device)
            ops.colsum_acc(g.view(-1, co), db)
        return dx, dw, db, None


def conv2d_same(x, weight, bias=None, relu=False, dilation=1):
    """NHWC convolution with padding="same", odd kernel, stride 1 and an optional dilation d.  The conv kernels have
    no dilation argument; a d-dilated convolution IS d*d ordinary convolutions on the pixel-parity sub-grids
    x[:, i::d, j::d] -> y[:, i::d, j::d] (each sub-grid sees its neighbours at distance d as adjacent; zero padding
    k // 2 on the sub-grid = d * (k // 2) on the image), so that is what runs -- exact, launch-heavy, and only used
    by the F2F baseline encoder (reference paper.py:245-261)."""
    x = x.contiguous()
    if dilation == 1:
        return ConvFn.apply(x, weight, bias, relu)
    B, H, W, _ = x.shape
    y = torch.empty((B, H, W, weight.shape[0]), dtype=x.dtype, device=x.device)
    parts = []
    for i in range(min(dilation, H)):
        for j in range(min(dilation, W)):
            parts.append((i, j, ConvFn.apply(x[:, i::dilation, j::dilation].contiguous(), weight, bias, relu)))
    return _ScatterGridFn.apply(y, dilation, *[t for _, _, t in parts])


class _ScatterGridFn(Function):
    """Interleave the d*d sub-grid results back into one image (parts ordered (i, j) row-major); the gradient of a
    part is the matching strided slice."""

    @staticmethod
    def forward(ctx, y, d, *parts):
        ctx.d = d
        k = 0
        H, W = y.shape[1], y.shape[2]
        for i in range(min(d, H)):
            for j in range(min(d, W)):
                y[:, i::d, j::d] = parts[k]
                k += 1
        return y

    @staticmethod
    def backward(ctx, g):
        d = ctx.d
        H, W = g.shape[1], g.shape[2]
        out = [g[:, i::d, j::d].contiguous() for i in range(min(d, H)) for j in range(min(d, W))]
        return (None, None) + tuple(out)


# ------------------------------------------------------------------------------------------------
# Dropout (train mode only; eval and p = 0 never reach these).  No mask tensor: the kernel hashes (seed, index),
# and the backward is the same call on the gradient.  Seeds advance with every call; data-parallel ranks are offset.
class _DropSeeds:
    def __init__(self):
        self.count = 0

    def next(self):
        self.count += 1
        rank = 0
        try:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized():
                rank = dist.get_rank()
        except Exception:
            rank = 0
        return mix64(torch.initial_seed() * 0x9E3779B97F4A7C15 + (rank << 40) + self.count)


def mix64(x):
    """splitmix64 finaliser.  The kernels hash (index ^ seed_lo) * C + seed_hi: seeds that differ only in their low
    word (a plain call counter) give masks that are index-XOR permutations of one another -- adjacent dropout sites
    and consecutive steps would share one mask up to a neighbour swap.  Every bit of the mixed seed depends on every
    bit of the counter, so consecutive calls differ in both words."""
    x &= 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return x ^ (x >> 31)


DROP_SEEDS = _DropSeeds()


def manual_seed(seed):
    """torch.manual_seed(seed) AND a restart of the dropout call counter (and of the device-side base captured steps
    advance): two trainings in ONE process draw the same masks only if both start here -- torch.manual_seed alone
    leaves the counter where the first training stopped.  A fresh process starts at zero by itself."""
    torch.manual_seed(seed)
    DROP_SEEDS.count = 0
    if ops.DROP_BASE is not None:
        ops.DROP_BASE.zero_()          # in place: captured graphs hold its address


class DropoutFn(Function):
    @staticmethod
    def forward(ctx, x, p, seed):
        ctx.p, ctx.seed = p, seed
        return ops.dropout(x, p, seed)

    @staticmethod
    def backward(ctx, g):
        return ops.dropout(g.contiguous(), ctx.p, ctx.seed), None, None


def dropout(x, p, training):
    """nn.Dropout(p)(x) semantics: identity unless `training` and p > 0."""
    if not training or p <= 0.0:
        return x
    return DropoutFn.apply(x.contiguous(), float(p), DROP_SEEDS.next())


# FOD_ATTN_FP8: fp8 attention (BASELINE.json configs[4], csrc/attention_fp8.hip).  "off": bf16 / f32 kernels everywhere;
# "long": the launches the block-shared LDS kernels take in bf16 (long query sequences: the encoder's self-attention,
# the joint encoders) run the MX-fp8 forward; "all": every bf16 attention without active dropout does (the decoder's
# few-query launches then lose their key split across blocks: slower, kept for tests and the record).
# The environment gives the start value; an explicit runs/_model.build_model(attn_dtype=...) / bench.py --attn-dtype
# overwrites it.
def _fp8_takes(q1, k1, drop_p):
    mode = SW.FOD_ATTN_FP8
    if mode == "off" or q1.dtype != torch.bfloat16 or drop_p > 0.0:
        return False
    few_queries = q1.shape[1] <= 512 and k1.shape[1] >= 128       # launch_all()'s split predicate (attention.hip)
    return mode == "all" or not few_queries


class AttentionFn(Function):
    @staticmethod
    def forward(ctx, q1, k1, v, q2, k2, scale, drop_p=0.0, drop_seed=0):
        ctx.drop = (drop_p, drop_seed)
        ctx.scale = scale
        ctx.two = q2 is not None
        ctx.fp8 = _fp8_takes(q1, k1, drop_p)
        if ctx.fp8:
            need_bwd = any(t is not None and t.requires_grad for t in (q1, k1, v, q2, k2))
            o, lse2, deq = ops.attn_fwd_fp8(q1, k1, v, scale, q2, k2, want_backward=need_bwd)
            if need_bwd:                 # the backward pass runs on the dequantised operands (same quantised scores)
                ctx.save_for_backward(deq[0], deq[1], deq[2], deq[3], deq[4], o, lse2)
            return o
        o, lse2 = ops.attn_fwd(q1, k1, v, scale, q2, k2, drop_p=drop_p, drop_seed=drop_seed)
        ctx.save_for_backward(q1, k1, v, q2, k2, o, lse2)
        return o

    @staticmethod
    def backward(ctx, do):
        q1, k1, v, q2, k2, o, lse2 = ctx.saved_tensors
        slots = {}
        qk = _column_siblings(q1, k1)
        if qk is not None:
            # q | k are the column halves of one buffer (InProjFn): dq | dk go out the same way
            D = q1.shape[-1]
            dqk = torch.empty_strided(qk.shape, qk.stride(), dtype=qk.dtype, device=qk.device)
            slots = dict(dq1_out=dqk[..., :D], dk1_out=dqk[..., D:])
        elif q1.shape == k1.shape == v.shape and q1.is_contiguous() and k1.is_contiguous() and v.is_contiguous():
            # self-attention: dq | dk | dv as consecutive blocks of one buffer, the layout a GroupLinearFn that
            # produced q, k, v takes as it is (no gather copies)
            buf = torch.empty((3,) + tuple(q1.shape), dtype=q1.dtype, device=q1.device)
            slots = dict(dq1_out=buf[0], dk1_out=buf[1], dv_out=buf[2])
        if ctx.fp8:
            # q was multiplied by scale * log2(e) before quantisation: scores = (1 / log2 e) q'.k, dq = scale log2(e) dq'
            dq1, dk1, dq2, dk2, dv = ops.attn_bwd(q1, k1, v, o, do.contiguous(), lse2, 1.0 / ops.LOG2E, q2, k2,
                                                  dq_scale=ctx.scale * ops.LOG2E, **slots)
            return dq1, dk1, dv, dq2, dk2, None, None, None
        dq1, dk1, dq2, dk2, dv = ops.attn_bwd(q1, k1, v, o, do.contiguous(), lse2, ctx.scale, q2, k2,
                                              drop_p=ctx.drop[0], drop_seed=ctx.drop[1], **slots)
        return dq1, dk1, dv, dq2, dk2, None, None, None


def _strided_ok(t):
    """A [B, T, E] operand the attention kernels take as it is: channel-contiguous, 16-byte strides / pointer."""
    v = _VEC[t.dtype]
    return (t.dim() == 3 and t.stride(-1) == 1 and t.stride(0) % v == 0 and t.stride(1) % v == 0
            and t.data_ptr() % 16 == 0)


def attention(q1, k1, v, scale, q2=None, k2=None, drop_p=0.0, training=False):
    """`drop_p` (with `training`): dropout on the attention probabilities, as MultiheadAttention(dropout=p)."""
    c = lambda t: None if t is None else (t if _strided_ok(t) else t.contiguous())
    drop = (float(drop_p), DROP_SEEDS.next()) if training and drop_p > 0.0 else ()
    return AttentionFn.apply(c(q1), c(k1), c(v), c(q2), c(k2), scale, *drop)


def _column_siblings(a, b):
    """a = buf[..., :D], b = buf[..., D:2D] of one [..., 2D] buffer?  Returns that buffer (a view) or None."""
    D = a.shape[-1]
    if (b is None or a.shape != b.shape or a.stride() != b.stride() or a.stride(-1) != 1 or a.stride(-2) != 2 * D
            or a.untyped_storage().data_ptr() != b.untyped_storage().data_ptr()
            or b.storage_offset() != a.storage_offset() + D):
        return None
    outer = 2 * D
    for n, st in zip(reversed(a.shape[:-1]), reversed(a.stride()[:-1])):      # dense apart from the column split
        if st != outer:
            return None
        outer *= n
    return torch.as_strided(a, tuple(a.shape[:-1]) + (2 * D,), a.stride())


class InProjFn(Function):
    """torch.nn.MultiheadAttention's packed input projection as the encoder uses it (reference
    transformer.py:401-411: q = k-input = src + pos, v-input = src): q | k from ONE GEMM over xp (N = 2D), v from
    one over src; the packed weight / bias get ONE gradient tensor each (no slice-and-accumulate kernels, and the
    same address every step).  q and k come back as the two column halves of one [.., 2D] buffer; the attention
    kernels read them strided and write dq | dk the same way."""

    @staticmethod
    def forward(ctx, xp, src, w, b):
        return _in_proj_forward(ctx, xp, src, w, b)

    @staticmethod
    def backward(ctx, dq, dk, dv):
        return _in_proj_backward(ctx, dq, dk, dv, ctx.needs_input_grad[0], ctx.needs_input_grad[1])


def _in_proj_forward(ctx, xp, src, w, b):
    """(q, k, v) of the packed projection: q | k = xp W_qk^T, v = src W_v^T."""
    D = w.shape[1]
    dtype = xp.dtype
    wqk, wv = prep_linear(w[:2 * D], dtype, False), prep_linear(w[2 * D:], dtype, False)
    qk = ops.gemm_nt(xp, wqk, shift=b[:2 * D]).view(*xp.shape[:-1], 2 * D)
    v = ops.gemm_nt(src, wv, shift=b[2 * D:]).view(src.shape)
    ctx.save_for_backward(xp, src)
    ctx.w, ctx.b = w, b
    return qk[..., :D], qk[..., D:], v


def _in_proj_backward(ctx, dq, dk, dv, need_xp, need_src, chained=False, dkeep=None):
    """(dxp, dsrc, dw, db) of the packed projection q | k = xp W_qk^T, v = src W_v^T.  `chained` (InProjSelfFn, where
    xp = src + pos): the residual path's gradient `dkeep` rides in the q | k input-gradient GEMM's epilogue and that
    result in the v one's, so dsrc is the whole gradient of src."""
    xp, src = ctx.saved_tensors
    w, b = ctx.w, ctx.b
    D = w.shape[1]
    dtype = xp.dtype
    rows = xp.numel() // D
    dqk = _column_siblings(dq, dk)
    if dqk is None:
        dqk = torch.cat([dq, dk], dim=-1)
    dqk = dqk.reshape(rows, 2 * D)
    dv = dv.contiguous().view(rows, D)
    dxp = dsrc = None
    if need_xp:
        res = None if dkeep is None else _grad_rows(dkeep, D, dtype)
        dxp = ops.gemm_nt(dqk, prep_linear(w[:2 * D], dtype, True), residual=res).view(xp.shape)
    if need_src:
        dsrc = ops.gemm_nt(dv, prep_linear(w[2 * D:], dtype, True), residual=dxp if chained else None).view(src.shape)
    dw = zeros_f32((3 * D, D), xp.device)
    db = zeros_f32((3 * D,), xp.device)
    wq = WGRADS.site((w, b))
    WGRADS.tn(wq, dqk, xp.view(rows, D), dw[:2 * D], db[:2 * D])
    WGRADS.tn(wq, dv, src.view(rows, D), dw[2 * D:], db[2 * D:])
    return dxp, dsrc, dw, db


def in_proj(xp, src, weight, bias):
    return InProjFn.apply(xp.contiguous(), src.contiguous(), weight, bias)


class InProjSelfFn(Function):
    """The encoder's self-attention input side as ONE autograd consumer of src: xp = src + pos, q | k = xp W_qk^T, v =
    src W_v^T, and src handed back for the residual step.  Separately, src has three consumers (the positional add,
    the v projection, the residual) and autograd sums their gradients with two kernels of its own per layer (14500 x 256
    elements each); here the residual gradient rides in the q | k input-gradient GEMM's epilogue and that result in the
    v one's.  `pos` (a table or per-frame tensor without gradient) is broadcast by the add kernel."""

    @staticmethod
    def forward(ctx, src, pos, w, b, row_mod):
        xp = ops.eltwise(L.EW_ADD, src, pos, b_row_mod=row_mod)
        return (src.view_as(src),) + _in_proj_forward(ctx, xp, src, w, b)

    @staticmethod
    def backward(ctx, dkeep, dq, dk, dv):
        need = ctx.needs_input_grad[0]
        _, dsrc, dw, db = _in_proj_backward(ctx, dq, dk, dv, need, need, chained=True, dkeep=dkeep)
        return dsrc, None, dw, db, None


def in_proj_self(src, pos, weight, bias):
    """-> (src for the residual step, q, k, v) with q = k-input = src + pos (see InProjSelfFn); None if `pos` carries a
    gradient or the fused form is switched off (the caller then takes the separate add + in_proj)."""
    if pos.requires_grad or not SW.FOD_LINEAR_KEEP:
        return None
    row_mod = pos.shape[-2] if pos.dim() == 2 else 0
    return InProjSelfFn.apply(src.contiguous(), pos.contiguous(), weight, bias, row_mod)


class InProjCrossFn(Function):
    """The packed input projection with three different inputs (encoder cross-attention onto the previous output /
    a previous frame, reference transformer.py:464-478: q-input = x + pos, k-input = other + pos, v-input = other).
    Three GEMMs; the packed weight / bias still get ONE gradient tensor each."""

    @staticmethod
    def forward(ctx, xq, xk, xv, w, b):
        D = w.shape[1]
        dtype = xq.dtype
        q = ops.gemm_nt(xq, prep_linear(w[:D], dtype, False), shift=b[:D]).view(xq.shape)
        k = ops.gemm_nt(xk, prep_linear(w[D:2 * D], dtype, False), shift=b[D:2 * D]).view(xk.shape)
        v = ops.gemm_nt(xv, prep_linear(w[2 * D:], dtype, False), shift=b[2 * D:]).view(xv.shape)
        ctx.save_for_backward(xq, xk, xv)
        ctx.w, ctx.b = w, b
        return q, k, v

    @staticmethod
    def backward(ctx, dq, dk, dv):
        xs = ctx.saved_tensors
        w, b = ctx.w, ctx.b
        D = w.shape[1]
        dtype = xs[0].dtype
        dw = zeros_f32((3 * D, D), xs[0].device)
        db = zeros_f32((3 * D,), xs[0].device)
        dxs = []
        wq = WGRADS.site((w, b))
        for i, (x, g) in enumerate(zip(xs, (dq, dk, dv))):
            rows = x.numel() // D
            g = g.contiguous().view(rows, D)
            sl = slice(i * D, (i + 1) * D)
            dxs.append(ops.gemm_nt(g, prep_linear(w[sl], dtype, True)).view(x.shape) if ctx.needs_input_grad[i] else None)
            WGRADS.tn(wq, g, x.view(rows, D), dw[sl], db[sl])
        return dxs[0], dxs[1], dxs[2], dw, db


def in_proj_cross(xq, xk, xv, weight, bias):
    return InProjCrossFn.apply(xq.contiguous(), xk.contiguous(), xv.contiguous(), weight, bias)


class RefPointSineFn(Function):
    """ref_logit [R,2] -> (ref f32 [R,2] = sigmoid, sine [R,D] ordered (y | x))."""

    @staticmethod
    def forward(ctx, ref_logit, D):
        ref, sine = ops.refpoint_sine_fwd(ref_logit, D)
        ctx.save_for_backward(ref)
        ctx.D, ctx.act_dtype = D, ref_logit.dtype
        return ref, sine

    @staticmethod
    def backward(ctx, dref, dsine):
        (ref,) = ctx.saved_tensors
        if dsine is None:
            dsine = torch.zeros((ref.shape[0], ctx.D), dtype=ctx.act_dtype, device=ref.device)
        return ops.refpoint_sine_bwd(dsine.contiguous(), ref, None if dref is None else dref.contiguous()), None


class BoxFinishFn(Function):
    """boxes f32 [L,R,4] = sigmoid(t + [inverse_sigmoid(ref[r % ref_rows]), 0, 0])."""

    @staticmethod
    def forward(ctx, t, ref, levels):
        boxes = ops.box_finish_fwd(t, ref, levels)
        ctx.save_for_backward(boxes, ref)
        ctx.act_dtype = t.dtype
        ctx.t_shape = t.shape
        return boxes

    @staticmethod
    def backward(ctx, dboxes):
        boxes, ref = ctx.saved_tensors
        dt_, dref = ops.box_finish_bwd(dboxes.contiguous(), boxes, ref, ctx.act_dtype)
        return dt_.view(ctx.t_shape), dref, None


class ZeroGradAnchor(Function):
    """Identity on `x`; gives the listed parameters an explicit all-zero gradient.

    Used for parameters whose gradient is identically zero by construction (projections that only
    feed the logits of a softmax over ONE key): the reference materialises zeros for them, and an
    optimizer with decoupled weight decay treats zero and None differently."""

    @staticmethod
    def forward(ctx, x, *params):
        ctx.shapes = [(p.shape, p.device) for p in params]
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return (g,) + tuple(zeros_f32(s, d) for s, d in ctx.shapes)


class CastFn(Function):
    """dtype conversion of a [*, cols] tensor with optional zero padding of the last dim; the gradient
    is converted back (and un-padded)."""

    @staticmethod
    def forward(ctx, x, dtype, pad_cols):
        ctx.src_dtype, ctx.cols = x.dtype, x.shape[-1]
        return cast(x, dtype, pad_cols)

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        cols = g.shape[-1]
        rows = g.numel() // cols
        out = ops.permute3_cast(g, ctx.src_dtype, (1, rows, ctx.cols), (0, cols, 1))
        return out.view(*g.shape[:-1], ctx.cols), None, None


def cast_ad(x, dtype, pad_cols=None):
    if x.dtype == dtype and pad_cols in (None, x.shape[-1]):
        return x
    return CastFn.apply(x.contiguous(), dtype, pad_cols)


# ------------------------------------------------------------------------------------------------
# Memory side of the decoder, hoisted out of the layer loop.
#
# The value / key_content projections of an image memory and the key_pos projection of the positional
# table do not depend on the decoder state, only on (memory, weights).  Instead of 2*L small GEMMs per
# image inside the layer loop (plus their 4*L backward GEMMs), every image gets ONE GEMM against the
# row-concatenated weights of all layers, the positional table gets ONE GEMM for all (layer, image)
# pairs, and each cross-attention reads / writes its [*, D] column slot of those wide buffers through
# the attention kernels' stride arguments.
# ------------------------------------------------------------------------------------------------


class WideLinearFn(Function):
    """y[*, P*D] = x[*, Din] @ cat_p(W_p)^T + cat_p(b_p): P Linear layers sharing one input, one GEMM.  An input without
    gradient (the positional table) gets none.  (A batch-shared table's gradient arrives already summed over the batch:
    HoistedCrossAttnFn does that before it hands the buffer on.)"""

    @staticmethod
    def forward(ctx, x, *params):
        P = len(params) // 2
        weights, biases = params[:P], params[P:]
        wcat, bcat, _ = CAT.get(weights, biases, x.dtype)
        y = ops.gemm_nt(x, wcat, shift=bcat).view(*x.shape[:-1], wcat.shape[0])
        ctx.save_for_backward(x)
        ctx.params = params
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        P = len(ctx.params) // 2
        weights, biases = ctx.params[:P], ctx.params[P:]
        D_out, D_in = weights[0].shape
        _, _, wcat_t = CAT.get(weights, biases, x.dtype)
        g = dy.contiguous().view(-1, P * D_out)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = ops.gemm_nt(g, wcat_t).view(x.shape)
        dw = zeros_f32((P * D_out, D_in), x.device)
        db = zeros_f32((P * D_out,), x.device)
        WGRADS.tn(WGRADS.site(ctx.params), g, x.view(-1, D_in), dw, db)
        gw = [dw[i * D_out:(i + 1) * D_out] for i in range(P)]
        gb = [db[i * D_out:(i + 1) * D_out] for i in range(P)]
        return (dx,) + tuple(gw) + tuple(gb)


class GroupLinearFn(Function):
    """P same-shaped Linear layers applied to ONE input, returned as P separate contiguous tensors (blocks of one
    [P, rows, D] buffer): one launch forward, one for the input gradient (the P output gradients are the k-segments
    of its A operand), one for all weight / bias gradients.  The decoder's query side is made of these: the
    self-attention's query_content / key_content / value, the per-image query_sine projections of a layer, and
    the per-layer projections of the learned query positions (reference transformer.py:66-70,139-141)."""

    @staticmethod
    def forward(ctx, x, nres, res_mod, *tensors):
        """`nres` > 0: the first nres of `tensors` are [R, D] tables (consecutive blocks of ONE buffer, as an earlier
        GroupLinearFn returns them) added to the first nres outputs in the launch's epilogue, row m + table[m % res_mod]
        -- the self-attention's q = q_content + q_pos, k = k_content + k_pos without their two element-wise launches."""
        res, params = tensors[:nres], tensors[nres:]
        P = len(params) // 2
        weights, biases = params[:P], params[P:]
        wcat, bcat, _ = CAT.get(weights, biases, x.dtype)
        D = weights[0].shape[0]
        rblock = None
        if nres:
            rblock = _as_segments(res, res[0].numel() // D, D)
            assert rblock is not None, "group_linear(residual=...): the tables must be consecutive blocks (the caller checks)"
        y = ops.group_linear_fwd(x.view(-1, x.shape[-1]), wcat, bcat, P, residual=rblock, res_row_mod=res_mod)
        ctx.save_for_backward(x)
        ctx.params, ctx.nres, ctx.res_mod, ctx.res_shape = params, nres, res_mod, (res[0].shape if nres else None)
        return tuple(y[p].view(*x.shape[:-1], D) for p in range(P))

    @staticmethod
    def backward(ctx, *gs):
        (x,) = ctx.saved_tensors
        P = len(ctx.params) // 2
        weights, biases = ctx.params[:P], ctx.params[P:]
        D, K = weights[0].shape
        _, _, wcat_t = CAT.get(weights, biases, x.dtype)
        rows = x.numel() // K
        g = _as_segments(gs, rows, D)
        if g is None:
            g = _gather_segments(gs, rows, D, x.dtype, x.device)
        dx = ops.group_linear_dgrad(g, wcat_t, P).view(x.shape) if ctx.needs_input_grad[0] else None
        dw = zeros_f32((P * D, K), x.device)
        db = zeros_f32((P * D,), x.device)
        WGRADS.grouped(WGRADS.site(ctx.params), g, x.view(rows, K), dw, db)
        dres = ()
        if ctx.nres:
            # the tables' gradients: the first nres output gradients summed over the rows that shared a table row
            dres = tuple((_sum_periodic(g[i], ctx.res_mod).view(ctx.res_shape) if ctx.res_mod and rows > ctx.res_mod
                          else g[i].view(ctx.res_shape)) if ctx.needs_input_grad[3 + i] else None for i in range(ctx.nres))
        return ((dx, None, None) + dres + tuple(dw[i * D:(i + 1) * D] for i in range(P))
                + tuple(db[i * D:(i + 1) * D] for i in range(P)))


def _as_segments(gs, rows, D):
    """The tensors of `gs` as one [P, rows, D] tensor if they already are consecutive contiguous blocks of one
    allocation (producers that know about the grouping write their gradients that way), else None."""
    g0 = gs[0]
    if g0 is None or not g0.is_contiguous() or g0.numel() != rows * D:
        return None
    st, step = g0.untyped_storage(), rows * D
    for p_, gp in enumerate(gs):
        if (gp is None or gp.dtype != g0.dtype or not gp.is_contiguous() or gp.numel() != step
                or gp.untyped_storage().data_ptr() != st.data_ptr()
                or gp.storage_offset() != g0.storage_offset() + p_ * step):
            return None
    return torch.as_strided(g0, (len(gs), rows, D), (step, D, 1))


def _gather_segments(gs, rows, D, dtype, device):
    """The gradients `gs` (None: zero) copied into one new [P, rows, D] tensor -- the segment layout: ONE launch."""
    g = torch.empty((len(gs), rows, D), dtype=dtype, device=device)
    dsts, srcs = [], []
    for p_, gp in enumerate(gs):
        if gp is None:
            g[p_].zero_()
        else:
            dsts.append(g[p_])
            srcs.append(gp.reshape(rows, D))
    if all(t.dtype == dtype and t.is_contiguous() for t in srcs):
        torch._foreach_copy_(dsts, srcs)     # (17 separate copies of 64 KB were 17 graph nodes of ~5 us each)
    else:
        for d_, s_ in zip(dsts, srcs):
            d_.copy_(s_)
    return g


def group_linear(x, linears, residual=None, res_row_mod=0):
    """[m(x) for m in linears] for nn.Linear-like holders of equal shape; grouped launches in bf16, plain
    per-layer launches otherwise (fp32 parity mode, odd widths).  `residual`: a list of [res_row_mod, D] tables added to
    the first len(residual) results, row m + table[m % res_row_mod] -- inside the launch when the tables are consecutive
    blocks of one buffer (what an earlier group_linear returns), as separate additions otherwise.  A table has exactly
    res_row_mod rows (the decoder's query positions): the gradient of a longer one would need zero rows behind the sum."""
    D, K = linears[0].weight.shape
    same = all(tuple(m.weight.shape) == (D, K) and m.bias is not None for m in linears)
    res = list(residual) if residual is not None else []
    assert not res_row_mod or all(r.shape[0] == res_row_mod for r in res), "group_linear(residual=...): tables of res_row_mod rows"
    if x.dtype != torch.bfloat16 or not same or D % 64 or K % 32 or len(linears) < 2:
        out = [linear(x, m.weight, m.bias) for m in linears]
        fused = False
    else:
        fused = bool(res) and SW.FOD_GROUP_RESIDUAL and all(r.dim() == 2 and r.shape[1] == D and r.dtype == x.dtype for r in res) \
            and _as_segments(res, res[0].shape[0], D) is not None and 0 < res_row_mod == res[0].shape[0]
        out = list(GroupLinearFn.apply(x.contiguous(), len(res) if fused else 0, res_row_mod if fused else 0,
                                       *(res if fused else []), *[m.weight for m in linears], *[m.bias for m in linears]))
    if res and not fused:
        for i, r in enumerate(res):
            out[i] = add(out[i], r, b_row_mod=res_row_mod)
    return out



class ImuBranchFn(Function):
    """The one-key IMU-token blocks of P transformer layers at once (EgodeepAttention.forward_single_key of every layer;
    reference transformer.py:108-119 with one key per frame, where softmax = 1 and the block reduces to
    value -> out_proj [-> norm1(o + o) -> MLP -> norm2]).  The blocks read only the IMU embedding `ego` [frames, D] -- not
    the layer's tokens -- so the P of them are independent: every step of the chain runs for all layers in ONE launch
    (fod_gemm_nt_grouped for the shared input, fod_gemm_nt_batched after it, the norms with per-layer parameter tables).
    Per layer that was 4 GEMMs + 2 norms forward and 4 + 2 + 2 backward on ~10 rows, each a ~5-9 us graph node.

    apply(ego, P, use_mlp, *params) with params = P value weights, P value biases, P out_proj weights, P biases and, with
    use_mlp, norm1 weights, biases, mlp[0] weights, biases, mlp[3] weights, biases, norm2 weights, biases (P each)
    -> P tensors [frames, D] (blocks of one buffer)."""

    @staticmethod
    def forward(ctx, ego, P, use_mlp, queue, *params):
        """`queue` (ResGradQueue or None): where the consumers of the P results leave their gradients' sums pending."""
        ctx.queue = queue
        groups = [params[i * P:(i + 1) * P] for i in range(len(params) // P)]
        wv, bv, wo, bo = groups[:4]
        M, D = ego.shape
        dtype = ego.dtype
        t = ops.group_linear_fwd(ego, *CAT.get(wv, bv, dtype)[:2], P)                       # [P, M, D]
        wo_cat, bo_cat, _ = CAT.get(wo, bo, dtype)
        o = ops.gemm_nt_batched(t, wo_cat, shift=bo_cat)
        saved = [ego, t]
        if use_mlp:
            g1, b1, w0, b0, w3, b3, g2, b2 = groups[4:]
            o2 = o.view(P * M, D)
            n1, s1, mean1, rstd1 = ops.layernorm_fwd(o2, STACK.get(g1), STACK.get(b1), residual=o2, group_rows=M)
            w0_cat, b0_cat, _ = CAT.get(w0, b0, dtype)
            h = ops.gemm_nt_batched(n1.view(P, M, D), w0_cat, shift=b0_cat, relu=True)      # [P, M, Dff]
            w3_cat, b3_cat, _ = CAT.get(w3, b3, dtype)
            y = ops.gemm_nt_batched(h, w3_cat, shift=b3_cat)
            e, s2, mean2, rstd2 = ops.layernorm_fwd(n1, STACK.get(g2), STACK.get(b2), residual=y.view(P * M, D),
                                                    group_rows=M)
            saved += [s1, mean1, rstd1, n1, h, s2, mean2, rstd2]
            e = e.view(P, M, D)
        else:
            e = o
        ctx.save_for_backward(*saved)
        ctx.P, ctx.use_mlp, ctx.params = P, use_mlp, params
        return tuple(e[p] for p in range(P))

    @staticmethod
    def backward(ctx, *gs):
        P, use_mlp, params = ctx.P, ctx.use_mlp, ctx.params
        groups = [params[i * P:(i + 1) * P] for i in range(len(params) // P)]
        wv, bv, wo, bo = groups[:4]
        saved = ctx.saved_tensors
        ego, t = saved[:2]
        M, D = ego.shape
        dtype, dev = ego.dtype, ego.device
        if ctx.queue is not None:
            ctx.queue.flush()                                # the slots handed out as gradients become real
        de = _as_segments(gs, M, D)
        if de is None or de.dtype != dtype:
            de = _gather_segments(gs, M, D, dtype, dev)

        def wgrads(ws, bs, g, x):
            """queued weight / bias gradients of P layers with their own inputs: g [P, M, N], x [P, M, K]"""
            N, K = ws[0].shape
            dw, db = zeros_f32((P * N, K), dev), zeros_f32((P * N,), dev)
            for p_ in range(P):
                WGRADS.tn(WGRADS.site((ws[p_], bs[p_])), g[p_], x[p_], dw[p_ * N:(p_ + 1) * N], db[p_ * N:(p_ + 1) * N])
            return [dw[p_ * N:(p_ + 1) * N] for p_ in range(P)], [db[p_ * N:(p_ + 1) * N] for p_ in range(P)]

        sl = lambda v: [v[p_ * D:(p_ + 1) * D] for p_ in range(P)]
        extra = []
        if use_mlp:
            g1, b1, w0, b0, w3, b3, g2, b2 = groups[4:]
            s1, mean1, rstd1, n1, h, s2, mean2, rstd2 = saved[2:]
            Dff = w0[0].shape[0]
            dg2, db2 = zeros_f32((P * D,), dev), zeros_f32((P * D,), dev)
            ds2 = ops.layernorm_bwd(de.view(P * M, D), s2, mean2, rstd2, STACK.get(g2), dg2, db2, group_rows=M)
            ds2 = ds2.view(P, M, D)                          # gradient of n1 + mlp(n1): the MLP output's and n1's residual share
            # the ReLU's gate rides in the epilogue of the GEMM that forms the hidden gradient
            dh = ops.gemm_nt_batched(ds2, CAT.get(w3, b3, dtype)[2], b_cols=True, relu_mask=h)          # [P, M, Dff]
            dw3, db3 = wgrads(w3, b3, ds2, h)
            dn1 = ops.gemm_nt_batched(dh, CAT.get(w0, b0, dtype)[2], b_cols=True, residual=ds2)         # + the residual path
            dw0, db0 = wgrads(w0, b0, dh, n1.view(P, M, D))
            dg1, db1 = zeros_f32((P * D,), dev), zeros_f32((P * D,), dev)
            ds1 = ops.layernorm_bwd(dn1.view(P * M, D), s1, mean1, rstd1, STACK.get(g1), dg1, db1, group_rows=M)
            do = ops.eltwise(L.EW_SCALE, ds1, alpha=2.0).view(P, M, D)       # norm1(o + o): o enters twice
            extra = sl(dg1) + sl(db1) + dw0 + db0 + dw3 + db3 + sl(dg2) + sl(db2)
        else:
            do = de
        dt_ = ops.gemm_nt_batched(do, CAT.get(wo, bo, dtype)[2], b_cols=True)                           # [P, M, D]
        dwo, dbo = wgrads(wo, bo, do, t)
        dego = ops.group_linear_dgrad(dt_, CAT.get(wv, bv, dtype)[2], P) if ctx.needs_input_grad[0] else None
        dwv, dbv = zeros_f32((P * D, D), dev), zeros_f32((P * D,), dev)
        WGRADS.grouped(WGRADS.site(tuple(wv) + tuple(bv)), dt_, ego, dwv, dbv)
        return (dego, None, None, None) + tuple(sl(dwv) + sl(dbv) + dwo + dbo + extra)


def imu_branch_fits(ego, blocks):
    """Whether the one-key IMU blocks `blocks` (EgodeepAttention-like holders) can run as ImuBranchFn: bf16, >= 2 same-shaped
    blocks with biases, widths inside the short-launch kernel's vector epilogue."""
    if not SW.FOD_IMU_BATCHED or len(blocks) < 2 or ego.dim() != 2 or ego.dtype != torch.bfloat16:
        return False
    D = ego.shape[1]
    b0 = blocks[0]
    for b in blocks:
        if b.use_mlp != b0.use_mlp:
            return False
        lins = [b.value, b.fun.out_proj] + ([b.mlp[0], b.mlp[3]] if b.use_mlp else [])
        if any(m.bias is None for m in lins):
            return False
        if tuple(b.value.weight.shape) != (D, D) or tuple(b.fun.out_proj.weight.shape) != (D, D):
            return False
        if b.use_mlp and (tuple(b.mlp[0].weight.shape) != tuple(b0.mlp[0].weight.shape)
                          or tuple(b.mlp[3].weight.shape) != (D, b0.mlp[0].weight.shape[0])):
            return False
    return D % 64 == 0 and (not b0.use_mlp or b0.mlp[0].weight.shape[0] % 64 == 0)


def imu_branch(ego, blocks, queue=None):
    """[block.forward_single_key(ego) without dropout for block in blocks] in a handful of launches (ImuBranchFn)."""
    P = len(blocks)
    use_mlp = blocks[0].use_mlp
    params = ([b.value.weight for b in blocks] + [b.value.bias for b in blocks]
              + [b.fun.out_proj.weight for b in blocks] + [b.fun.out_proj.bias for b in blocks])
    if use_mlp:
        params += ([b.norm1.weight for b in blocks] + [b.norm1.bias for b in blocks]
                   + [b.mlp[0].weight for b in blocks] + [b.mlp[0].bias for b in blocks]
                   + [b.mlp[3].weight for b in blocks] + [b.mlp[3].bias for b in blocks]
                   + [b.norm2.weight for b in blocks] + [b.norm2.bias for b in blocks])
    return list(ImuBranchFn.apply(ego.contiguous(), P, use_mlp, queue, *params))


def _sum_leading(t, n):
    """[n, ...] -> [...] : sum over the (tiny) leading dim."""
    acc = t[0]
    for i in range(1, n):
        acc = ops.eltwise(L.EW_ADD, acc.contiguous(), t[i].contiguous())
    return acc.contiguous()


def wide_linear(x, linears):
    ws = [m.weight for m in linears]
    bs = [m.bias for m in linears]
    return WideLinearFn.apply(x.contiguous(), *ws, *bs)


class MemorySide:
    """Per-forward holder of the hoisted projections and of the gradient buffers their slots are written to."""

    def __init__(self, big, ks_all, n_layers, n_images, D):
        self.big = big              # list over images: [B, N, 2*L*D]  (per layer: [value | key_content])
        self.ks_all = ks_all        # [N, L*K*D]                         (per (layer, image): key_pos(pos))
        self.L, self.K, self.D = n_layers, n_images, D
        self.dbig = [None] * n_images
        self.dks = None
        self.dq2 = {}

    def slots(self, layer, image):
        D = self.D
        b = self.big[image]
        v = b[..., (2 * layer) * D:(2 * layer + 1) * D]
        kc = b[..., (2 * layer + 1) * D:(2 * layer + 2) * D]
        q = layer * self.K + image
        ks = self.ks_all[..., q * D:(q + 1) * D]      # [N, D] table shared by the batch, or [B, N, D] (temporal term)
        return kc, ks, v


class _DkvQueue:
    """The dk / dv passes of the decoder's cross-attention blocks (one per layer and image: 30 per step) wait here during the
    backward sweep and run as ONE launch (fod_attn_bwd_dkv_multi; 32 jobs at most per launch) when the first consumer of
    their results is reached: each writes its own (layer, image) slot of MemorySide.dbig / .dks, which nothing reads
    before the call that hands the buffers to autograd (layer 0)."""

    def __init__(self):
        self.jobs, self.key, self.shp = [], None, None

    def push(self, key, shp, job):
        if self.jobs and (key != self.key or len(self.jobs) == 32):
            self.flush()
        self.key, self.shp = key, shp
        self.jobs.append(job)

    def flush(self):
        if self.jobs:
            jobs, self.jobs = self.jobs, []
            ops.attn_bwd_dkv_multi(jobs, self.shp)


class HoistedCrossAttnFn(Function):
    """softmax((q1.kc + q2.ks) * scale) v with kc / v / ks taken as column slots of the hoisted buffers.
    Gradients of the slots are written in place into MemorySide.dbig / .dks; the buffers are handed to
    autograd once, by the call that runs LAST in the backward sweep (layer 0; image 0 for ks), when every
    slot has been filled -- all earlier (higher-layer) calls return None for them."""

    @staticmethod
    def forward(ctx, q1, q2, big_j, ks_all, side, layer, image, scale, drop_p=0.0, drop_seed=0):
        kc, ks, v = side.slots(layer, image)
        o, lse2 = ops.attn_fwd(q1, kc, v, scale, q2, ks, drop_p=drop_p, drop_seed=drop_seed)
        ctx.save_for_backward(q1, q2, o, lse2)
        ctx.side, ctx.layer, ctx.image, ctx.scale = side, layer, image, scale
        ctx.drop = (drop_p, drop_seed)
        return o

    @staticmethod
    def backward(ctx, do):
        q1, q2, o, lse2 = ctx.saved_tensors
        side, layer, image, D = ctx.side, ctx.layer, ctx.image, ctx.side.D
        kc, ks, v = side.slots(layer, image)
        if side.dbig[image] is None:
            side.dbig[image] = torch.empty_like(side.big[image])
        per_batch_pos = side.ks_all.dim() == 3
        if side.dks is None:
            B = q1.shape[0]
            shape = tuple(side.ks_all.shape) if per_batch_pos else (B,) + tuple(side.ks_all.shape)
            side.dks = torch.empty(shape, dtype=side.ks_all.dtype, device=q1.device)
        db = side.dbig[image]
        dv = db[..., (2 * layer) * D:(2 * layer + 1) * D]
        dkc = db[..., (2 * layer + 1) * D:(2 * layer + 2) * D]
        qi = layer * side.K + image
        dks = side.dks[..., qi * D:(qi + 1) * D]
        # dq2 of the K images of a layer as consecutive blocks (their query_sine projections are one GroupLinearFn)
        key = (layer, tuple(q2.shape))
        if key not in side.dq2:
            side.dq2[key] = torch.empty((side.K,) + tuple(q2.shape), dtype=q2.dtype, device=q2.device)
        B_, Tq_, S_ = q1.shape[0], q1.shape[1], kc.shape[1]
        if (SW.FOD_DKV_QUEUE and q1.dtype == torch.bfloat16 and ctx.drop[0] == 0.0 and Tq_ <= 512 and S_ >= 256
                and dks.dim() == 3):
            # (the few-query shapes: what fod_attn_bwd would run as dq + attn_bwd_dkv_pf_kernel; the same kernel body runs
            # the queued jobs, so the results are bit-equal)
            do_c = do.contiguous()
            dq1, dq2, delta, shp = ops.attn_bwd_dq(q1, kc, v, o, do_c, lse2, ctx.scale, q2, ks, dk2_like=dks,
                                                   dq2_out=side.dq2[key][image])
            if getattr(side, "dkv_queue", None) is None:
                side.dkv_queue = _DkvQueue()
            qkey = (tuple(q1.shape), q1.stride(), kc.stride(), v.stride(), ks.stride(), dks.stride(), tuple(kc.shape),
                    float(ctx.scale))
            side.dkv_queue.push(qkey, shp, (q1, q2, kc, ks, v, do_c, lse2, delta, dkc, dks, dv))
            if layer == 0:
                side.dkv_queue.flush()                  # this call hands dbig[image] (and, at image 0, dks) on
        else:
            if getattr(side, "dkv_queue", None) is not None:
                side.dkv_queue.flush()
            dq1, _, dq2, _, _ = ops.attn_bwd(q1, kc, v, o, do.contiguous(), lse2, ctx.scale, q2, ks,
                                             dk1_out=dkc, dv_out=dv, dk2_out=dks, dq2_out=side.dq2[key][image],
                                             drop_p=ctx.drop[0], drop_seed=ctx.drop[1])
        g_big = side.dbig[image] if layer == 0 else None
        # a batch-shared ks_all gets the sum of the per-batch slots
        g_ks = None
        if layer == 0 and image == 0:
            g_ks = side.dks if per_batch_pos else _sum_leading(side.dks, side.dks.shape[0])
        return dq1, dq2, g_big, g_ks, None, None, None, None, None, None


def hoisted_cross_attention(q1, q2, side, layer, image, scale, drop_p=0.0, training=False):
    drop = (float(drop_p), DROP_SEEDS.next()) if training and drop_p > 0.0 else ()
    return HoistedCrossAttnFn.apply(q1.contiguous(), q2.contiguous(), side.big[image], side.ks_all, side, layer,
                                    image, scale, *drop)
