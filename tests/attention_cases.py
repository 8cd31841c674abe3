"""Attention problems whose float64 softmax is the TRUE answer of what the kernels compute, with a countable error budget.

Every attention kernel forms c = scale * log2(e) in f32; the LDS family rounds c * q to bf16.  With scale = ln(2) / 8 the f32
product is exactly 0.125, so integer queries |q| <= 256 give bf16(c * q) = q / 8 bit for bit, and with integer keys every
score is an exact multiple of 1/8 (log2 units) in any f32 accumulator of any kernel family.  What the kernels then lose
is countable: the bf16 probability tile, the bf16 dS tile, a normaliser summed from rounded probabilities, delta taken
from the rounded output, the result.  Each is a RELATIVE error of one term, so the tolerance of an element is a small
multiple of u = 2^-8 times the SUM OF MAGNITUDES of that element's terms (the companion `A`), not a norm and not sqrt(S).

Three operand profiles (pure torch on the CPU, float64 throughout, importable without a GPU):

  pointer  keys carry the one-hot hex digits of their class (two neighbouring keys share a class and tie exactly; with one
           part classes 256 apart tie too, across distant tiles; part 2 repeats the low digit and carries the third, each
           weighted 2 bits), a query puts 8 A on one low digit and 8 Bq on one high digit (A in {4, 8}, Bq in {4, 8, 24}
           bits): one class scores A + Bq bits, about thirty keys A or Bq, the rest 0.  Jumps of 4 bits stay under the
           LDS forward's 2^6 deferred-rescale threshold, 8 / 12 / 32 cross it.  Every key also carries a -1 marker on a
           digit its own queries do not look at, so the keys of a class differ in dq.  The keys of a pair have values of
           opposite sign in every channel and dout lives on two channels per query, signed with the first key's value:
           no element is a sum of cancelling terms, so one lost, doubled or misplaced key or query row stands far above
           the budget.  Calls 2 n and 2 n + 1 share a target map that shifts with n until every class has been some
           query's target and every query row has owned two channels of its target's dv; the odd call keeps to A = 8,
           Bq in {8, 24} and 8 bits on the third digit, so every key is also the target of a query to which nothing
           else matters (2 calls where Tq covers the classes, 12 for 128 x 1450, 62 for 33 x 2000).
  flat     q = 0: every probability is exactly 1 / S, the running maximum never moves, dk is exactly 0; k and v are a
           constant on the aligned 32-key runs that feed a channel and 0 elsewhere, dout lives on four channels of one
           parity per query, so a missing tile empties or halves its channels.
  dropout  the pointer profile under drop_p = 0.5 (1 / keep = 2 exactly) with the kernels' keep hash restated in numpy.

attend64() is the one float64 restatement (explicit gradients, key weights and query-row weights for the mutants and the
leave-one-out conditions); the reference gradients of a problem come from autograd and are held against it.
"""
import functools
import math
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

import variant_cases as V
from test_kernels_gpu import FP8_SHAPES, _drop_keep_mask

LN2 = math.log(2.0)
SCALE = LN2 / 8.0                       # the `scale` argument: f32(SCALE) * f32(log2 e) == 0.125 exactly
NAT = 0.125 * LN2                       # d(natural-log score) / d(q . k)
DROP_P = 0.5
U = 2.0 ** -8                           # bf16 unit roundoff as the budgets count it
PASSES = ("o", "dq1", "dk1", "dv", "dq2", "dk2")
# per-element bounds: factor * A (lse2: absolute, log2 units)
FACTOR = {"bf16": dict(o=4 * U, dv=4 * U, dq1=8 * U, dk1=8 * U, dq2=8 * U, dk2=8 * U, lse2=2.0 ** -8),
          "f32": dict(o=2e-5, dv=2e-5, dq1=2e-5, dk1=2e-5, dq2=2e-5, dk2=2e-5, lse2=2.0 ** -10)}
FP8_FACTOR = dict(o=2.0 ** -4 + 2.0 ** -6, lse2=2.0 ** -3)
DETECT = 8.0                            # a removed key / row moves some element by this many tolerances (fp8 forward: 2)

Problem = namedtuple("Problem", "shape profile call q1 k1 v q2 k2 dout drop seed ref A")


def exact_scale_products():
    """c = f32(scale) * f32(log2 e) for scale = ln 2 / 4, / 8, / 16."""
    return [float(np.float32(LN2 / d) * np.float32(1.4426950408889634)) for d in (4.0, 8.0, 16.0)]


def heads(t, H):
    return t.view(t.shape[0], t.shape[1], H, 32).transpose(1, 2)          # [B, H, T, 32]


def unheads(t):
    B, H, T, _ = t.shape
    return t.transpose(1, 2).reshape(B, T, H * 32)


# ------------------------------------------------------------------------------------------------ the float64 restatement
def attend64(p, w=None, rw=None, dout=None, internals=False, scale=None):
    """Attention and its gradients on the problem's operands in float64, explicit formulas.  w [B,H,Tq,S] (broadcastable):
    weight of key s in the softmax sums of query i (0 = removed, 2 = counted twice); rw [B,H,Tq,1]: weight of query row
    i in the dk / dv sums; dout: another upstream gradient; scale: another softmax scale than ln 2 / 8 (the Gaussian
    problems of the other tests).  -> dict of o, lse2 and the gradients ([B,T,E] / [B,H,Tq])."""
    B, H, Tq, S, parts = p.shape
    d = lambda t: None if t is None else heads(t.double(), H)
    Q1, K1, Vh, Q2, K2 = d(p.q1), d(p.k1), d(p.v), d(p.q2), d(p.k2)
    DO = d(p.dout if dout is None else dout)
    s2 = Q1 @ K1.transpose(-1, -2)
    if parts == 2:
        s2 = s2 + Q2 @ K2.transpose(-1, -2)
    c2, nat = (0.125, NAT) if scale is None else (scale / LN2, scale)
    s2 = s2 * c2
    m = s2.max(-1, keepdim=True).values
    e = torch.exp2(s2 - m)
    if w is not None:
        e = e * w
    Z = e.sum(-1, keepdim=True)
    P = e / Z
    g = keep_gain(p)
    Pd = P if g is None else P * g
    o = Pd @ Vh
    dP = DO @ Vh.transpose(-1, -2)
    if g is not None:
        dP = dP * g
    delta = (DO * o).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    dSr, Pdr = (dS, Pd) if rw is None else (dS * rw, Pd * rw)
    out = dict(o=unheads(o), lse2=(m + torch.log2(Z)).squeeze(-1), dq1=unheads(nat * (dS @ K1)),
               dk1=unheads(nat * (dSr.transpose(-1, -2) @ Q1)), dv=unheads(Pdr.transpose(-1, -2) @ DO))
    if parts == 2:
        out["dq2"] = unheads(nat * (dS @ K2))
        out["dk2"] = unheads(nat * (dSr.transpose(-1, -2) @ Q2))
    if internals:
        out["_"] = SimpleNamespace(P=P, Pd=Pd, g=g, dP=dP, dS=dS, o=o, delta=delta, Q1=Q1, K1=K1, V=Vh, Q2=Q2, K2=K2, DO=DO)
    return out


def keep_gain(p):
    """keep / (1 - drop_p) of the problem's dropout call ([B,H,Tq,S] float64), None without dropout."""
    if not p.drop:
        return None
    B, H, Tq, S, _ = p.shape
    return _drop_keep_mask(B, H, Tq, S, p.seed, p.drop).double() / (1.0 - p.drop)


def _autograd_reference(shape, ops_, dout, g):
    """(o, lse2, grads) of softmax(0.125 * (q1.k1 + q2.k2) * ln 2) [* g] v by float64 autograd."""
    B, H, Tq, S, parts = shape
    leaves = [None if t is None else t.double().requires_grad_(True) for t in ops_]
    q1, k1, v, q2, k2 = (None if t is None else heads(t, H) for t in leaves)
    s = q1 @ k1.transpose(-1, -2)
    if parts == 2:
        s = s + q2 @ k2.transpose(-1, -2)
    s = s * 0.125
    P = torch.softmax(s * LN2, dim=-1)
    if g is not None:
        P = P * g
    o = unheads(P @ v)
    o.backward(dout.double())
    lse2 = torch.logsumexp(s.detach() * LN2, -1) / LN2
    return o.detach(), lse2, [None if t is None else t.grad for t in leaves]


def _companions(p, r):
    """The sum of magnitudes of the terms of every element (module docstring): A_o = P|v|, A_dv = P^T|dO|,
    M = P (|dO||v|^T + rowsum(|dO||o|)), A_dq = scale M|k|, A_dk = scale M^T|q|."""
    i = r["_"]
    aDO, aV = i.DO.abs(), i.V.abs()
    M = i.Pd * (aDO @ aV.transpose(-1, -2)) + i.P * (aDO * i.o.abs()).sum(-1, keepdim=True)
    A = dict(o=unheads(i.Pd @ aV), dv=unheads(i.Pd.transpose(-1, -2) @ aDO), dq1=unheads(NAT * (M @ i.K1.abs())),
             dk1=unheads(NAT * (M.transpose(-1, -2) @ i.Q1.abs())))
    if i.Q2 is not None:
        A["dq2"] = unheads(NAT * (M @ i.K2.abs()))
        A["dk2"] = unheads(NAT * (M.transpose(-1, -2) @ i.Q2.abs()))
    return A


# ------------------------------------------------------------------------------------------------ operand layouts
Layout = namedtuple("Layout", "ncls smod groups ncalls")


def layout(shape):
    """Pointer profile: classes of neighbouring keys (a last odd key joins the pair before it), how many of them a query
    can tell apart (one part: classes 256 apart tie), how many queries share a target, and the number of calls after
    which every class has been a target and every query row has owned two dout channels of its target."""
    B, H, Tq, S, parts = shape
    ncls = max(S // 2, 1)
    smod = min(ncls, 256) if parts == 1 else ncls
    groups = -(-Tq // smod)
    return Layout(ncls, smod, groups, max(-(-smod // Tq), -(-groups // 16)))


def n_calls(shape, profile):
    return 1 if profile == "flat" else 2 * layout(shape).ncalls


def _key_class(shape):
    S = shape[3]
    return torch.clamp(torch.arange(S) // 2, max=max(S // 2 - 1, 0))


def _pointer_operands(shape, call_index):
    """Calls 2 n and 2 n + 1 share the target map: the even one cycles A / Bq over every pair of {4, 8} x {4, 8, 24}, the
    odd one keeps to {8} x {8, 24} and weights the third digit 8 bits, so that every class is also the target of a query
    to which nothing else matters (what the dq pass loses with a key stands alone there)."""
    B, H, Tq, S, parts = shape
    lay = layout(shape)
    call, strong = call_index // 2, call_index % 2 == 1
    gen = torch.Generator().manual_seed(7919 * call_index + 13)
    b_ix, h_ix = torch.arange(B).view(B, 1, 1), torch.arange(H).view(1, H, 1)
    off = 3 * h_ix + 5 * b_ix + 7 * call_index                                     # [B, H, 1]
    cls0 = _key_class(shape)                                                        # [S]
    kcls = cls0.view(1, 1, S) + off                                                 # [B, H, S]
    s_ix = torch.arange(S).view(1, 1, S).expand(B, H, S)
    k1 = torch.zeros(B, H, S, 32)
    k1.scatter_(-1, (kcls % 16).unsqueeze(-1), 1.0)
    k1.scatter_(-1, (16 + (kcls // 16) % 16).unsqueeze(-1), 1.0)
    k2 = torch.zeros(B, H, S, 32)
    k2.scatter_(-1, ((kcls // 256) % 16).unsqueeze(-1), 1.0)
    k2.scatter_(-1, (16 + kcls % 16).unsqueeze(-1), 1.0)
    # every key of a class carries a marker of -1 4, 8 or 12 low digits away: its own queries do not look there (the tie
    # stays exact), dq tells the keys of a class apart, and the queries of that digit score it A bits LOWER (never a
    # second full match)
    member = (torch.arange(S) - 2 * cls0).view(1, 1, S, 1)                          # 0, 1 (, 2 for a last odd key)
    marker = ((kcls.unsqueeze(-1) + 4 * (member + 1)) % 16)
    k1.scatter_(-1, marker, -1.0)
    k2.scatter_(-1, 16 + marker, -1.0)
    # queries: target class u, weights A / Bq bits on its low / high digit, 2 bits on the third (part 2)
    i = torch.arange(Tq)
    u = (i + call * Tq) % lay.smod                                                  # [Tq]
    grp = i // lay.smod
    active = torch.ones(Tq, dtype=torch.bool) if lay.groups <= 16 else (grp // 16 == call % -(-lay.groups // 16))
    a_bits = torch.tensor([8.0, 8.0] if strong else [4.0, 8.0])[((i + call) // 5) % 2]
    b_bits = torch.tensor([8.0, 24.0, 24.0] if strong else [4.0, 8.0, 24.0])[((i + call) // 2) % 3]
    tcls = u.view(1, 1, Tq) + off                                                   # [B, H, Tq]
    q1 = torch.zeros(B, H, Tq, 32)
    q1.scatter_(-1, (tcls % 16).unsqueeze(-1), (8 * a_bits).view(1, 1, Tq, 1).expand(B, H, Tq, 1))
    q1.scatter_(-1, (16 + (tcls // 16) % 16).unsqueeze(-1), (8 * b_bits).view(1, 1, Tq, 1).expand(B, H, Tq, 1))
    q2 = torch.zeros(B, H, Tq, 32)
    q2.scatter_(-1, ((tcls // 256) % 16).unsqueeze(-1), 64.0 if strong else 16.0)
    q2.scatter_(-1, (16 + tcls % 16).unsqueeze(-1), 16.0)
    # values: magnitudes 1..7, signs alternate inside a class (tied classes of a one-part case share the pattern)
    mag = torch.randint(1, 8, (B, H, S, 32), generator=gen).float()
    sign_key = cls0 % 256 if parts == 1 else cls0
    base = (torch.randint(0, 2, (B, H, int(sign_key.max()) + 1, 32), generator=gen) * 2 - 1).float()
    v = mag * base[:, :, sign_key] * (1 - 2 * (member % 2)).float()
    # dout: two channels per query, chosen by its group and target, signed so that its two terms add up and that the
    # queries of one target pull the same way
    sig = (1 - 2 * (u % 2)).float().view(1, 1, Tq).expand(B, H, Tq)
    dmag = torch.randint(1, 4, (B, H, Tq, 2), generator=gen).float()
    dout = torch.zeros(B, H, Tq, 32)
    first = torch.clamp(2 * u, max=S - 1)                                           # the class's first key
    for r in range(2):
        ch = ((2 * (grp % 16) + r + 3 * u) % 32).view(1, 1, Tq, 1).expand(B, H, Tq, 1)
        vsign = torch.sign(v[:, :, first].gather(-1, ch))
        dout.scatter_(-1, ch, (dmag[..., r:r + 1] * sig.unsqueeze(-1) * vsign))
    dout = dout * active.float().view(1, 1, Tq, 1)
    two = parts == 2
    return (unheads(q1), unheads(k1), unheads(v), unheads(q2) if two else None, unheads(k2) if two else None, unheads(dout))


def flat_units(S):
    """Flat profile: (unit of key s, number of units, hot [S, 32]).  A unit is an aligned run of 32 keys (one key below 64
    keys); unit r feeds the channels c with c % min(units, 32) == r % 32, where k and v are a constant and 0 elsewhere:
    a missing run empties or halves its channels."""
    s = torch.arange(S)
    unit = s // 32 if S >= 64 else s
    n = int(unit.max()) + 1
    hot = (torch.arange(32).view(1, 32) % min(n, 32) == (unit % 32).view(S, 1)).float()
    return unit, n, hot


def _flat_operands(shape, call):
    B, H, Tq, S, parts = shape
    gen = torch.Generator().manual_seed(104729 + call)
    hot = flat_units(S)[2]
    c_ix, h_ix = torch.arange(32).view(1, 1, 1, 32), torch.arange(H).view(1, H, 1, 1)
    vconst = (1 + (c_ix + h_ix) % 7).float() * (1 - 2 * (c_ix % 2)).float()
    v = (hot.view(1, 1, S, 32) * vconst).expand(B, H, S, 32)
    k1 = (hot.view(1, 1, S, 32) * (1 + (c_ix + 2 * h_ix) % 5).float()).expand(B, H, S, 32)
    k2 = (hot.view(1, 1, S, 32) * (1 + (2 * c_ix + h_ix) % 3).float()).expand(B, H, S, 32)
    q = torch.zeros(B, Tq, H * 32)
    # dout: 1..3 on four channels per query (i + 8 r: one parity, so the terms of delta share a sign)
    on = ((c_ix.view(1, 32) - torch.arange(Tq).view(Tq, 1)) % 8 == 0).float()          # [Tq, 32]
    dout = unheads(torch.randint(1, 4, (B, H, Tq, 32), generator=gen).float() * on.view(1, 1, Tq, 32))
    two = parts == 2
    return (q, unheads(k1), unheads(v), q.clone() if two else None, unheads(k2) if two else None, dout)


@functools.lru_cache(maxsize=64)
def problem(shape, profile, call=0):
    """Operands (float32 tensors holding integers), the float64 reference and the companions of one call; shared by the
    cases that run the shape one after the other (runs() is sorted by shape), nobody writes to what this returns."""
    q1, k1, v, q2, k2, dout = (_flat_operands if profile == "flat" else _pointer_operands)(shape, call)
    drop = DROP_P if profile == "dropout" else 0.0
    seed = (0x1234567890ABCDEF + 0x9E3779B97F4A7C15 * call) & 0xFFFFFFFFFFFFFFFF if drop else 0
    p = Problem(shape, profile, call, q1, k1, v, q2, k2, dout, drop, seed, None, None)
    r = attend64(p, internals=True)
    o, lse2, grads = _autograd_reference(shape, (q1, k1, v, q2, k2), dout, r["_"].g)
    ref = dict(o=o, lse2=lse2, dq1=grads[0], dk1=grads[1], dv=grads[2])
    if shape[4] == 2:
        ref.update(dq2=grads[3], dk2=grads[4])
    for name, want in ref.items():                                    # the explicit formulas are the autograd's
        assert float((r[name] - want).abs().max()) <= 1e-12 * (1.0 + float(want.abs().max())), (shape, profile, call, name)
    return p._replace(ref=ref, A=_companions(p, r))


def with_internals(p):
    """attend64 of the problem with its intermediate tensors (not cached: they are large)."""
    return attend64(p, internals=True)


# ------------------------------------------------------------------------------------------------ bounds
def violations(p, got, dtype, factors=None, passes=None, extra=None):
    """[(pass, worst err / bound, (b, token, head, channel) of the first bad element or None)] of results `got` (a dict of
    CPU tensors by pass name) against the problem's reference.  Where A is 0 the result must be 0; no element is exempt.
    extra: {pass: tensor} added to the bound (fp8_backward_extra)."""
    f = FACTOR[dtype] if factors is None else factors
    out = []
    for name in (passes or [n for n in ("o", "lse2") + PASSES[1:] if n in p.ref and n in got]):
        ref, have = p.ref[name], got[name].double()
        err = (have - ref).abs()
        bound = torch.full_like(ref, f[name]) if name == "lse2" else f[name] * p.A[name]
        if extra is not None and name in extra:
            bound = bound + extra[name]
        bad = (err > bound) | ~torch.isfinite(have)
        ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
        where = None
        if bool(bad.any()):
            idx = [int(x) for x in np.unravel_index(int(torch.nonzero(bad.flatten())[0]), bad.shape)]
            where = (idx[0], idx[2], idx[1], None) if name == "lse2" else (idx[0], idx[1], idx[2] // 32, idx[2] % 32)
        out.append((name, float(ratio.max()), where))
    return out


def assert_within(p, got, dtype, what, factors=None, passes=None, extra=None):
    """Every pass inside its bound, or a message naming the pass, the first bad (b, token, head, channel) and `what`
    (case id and route).  -> {pass: worst err / bound}."""
    res = violations(p, got, dtype, factors, passes, extra)
    bad = [(n, f"{r:.3g} x bound", f"first bad (b, token, head, channel) = {w}") for n, r, w in res if w is not None]
    assert not bad, f"{what} [{p.profile} call {p.call}]: {bad}"
    return {n: r for n, r, _ in res}


def fp8_backward_extra(p):
    """What the bf16 backward inherits when the forward was the fp8 one.  The fp8 forward stores p 2^4 in e4m3 relative to a
    running maximum that trails the true one by at most 4 bits (csrc/attention_fp8.hip:28-29 and the `pack4(ex2f(...))`
    tile): probabilities of these profiles are powers of two (integer scores in bits) and are held exactly down to 2^-13
    of the row's largest (e4m3's smallest subnormal is 2^-9); smaller ones are rounded to that grid or flushed, so the
    normaliser -- and with it lse2 -- may be off by their mass phi = sum of P below 2^-13 of the row's maximum, and o by
    2 phi A_o.  The backward forms
    P = exp2(score - lse2): every probability of the row is off by eps = phi / (1 - phi) relative, delta by
    sum_c |dO| 2 phi A_o.  -> {pass: tensor} to add to the bf16 bounds: dv (eps Pd)^T |dO|; dq / dk from
    M' = eps M + P sum_c |dO| 2 phi A_o."""
    i = attend64(p, internals=True)["_"]
    H = p.shape[1]
    small = i.P < i.P.max(-1, keepdim=True).values * 2.0 ** -13
    phi = (i.P * small).sum(-1, keepdim=True)
    eps = phi / (1.0 - phi)
    aDO, aV = i.DO.abs(), i.V.abs()
    M = i.Pd * (aDO @ aV.transpose(-1, -2)) + i.P * (aDO * i.o.abs()).sum(-1, keepdim=True)
    Me = eps * M + i.P * (aDO * 2.0 * phi * (i.Pd @ aV)).sum(-1, keepdim=True)
    out = dict(dv=unheads((eps * i.Pd).transpose(-1, -2) @ aDO), dq1=unheads(NAT * (Me @ i.K1.abs())),
               dk1=unheads(NAT * (Me.transpose(-1, -2) @ i.Q1.abs())))
    if i.Q2 is not None:
        out.update(dq2=unheads(NAT * (Me @ i.K2.abs())), dk2=unheads(NAT * (Me.transpose(-1, -2) @ i.Q2.abs())))
    return out


# ------------------------------------------------------------------------------------------------ the roundings, emulated
def rb(x):
    return x.float().bfloat16().double()


def emulate_bf16(p, lds):
    """The countable roundings of the bf16 kernels applied to the float64 computation: the probability tile, the normaliser
    (summed from the rounded tile in the LDS forward, from the unrounded one elsewhere), the output, delta from the rounded
    output, P from the forward's own lse2, the dS tile, the f32 scale, the results."""
    i = with_internals(p)["_"]
    B, H, Tq, S, parts = p.shape
    s2 = (i.Q1 @ i.K1.transpose(-1, -2) + (i.Q2 @ i.K2.transpose(-1, -2) if parts == 2 else 0.0)) * 0.125
    m = s2.max(-1, keepdim=True).values
    e = torch.exp2(s2 - m)
    g = 1.0 if i.g is None else i.g
    Pt = rb(e * g)
    l = rb(e).sum(-1, keepdim=True) if lds else e.sum(-1, keepdim=True)
    o = rb((Pt @ i.V) / l)
    lse2 = (m + torch.log2(l)).float().double()
    Pb = torch.exp2(s2 - lse2)
    delta = (i.DO * o).sum(-1, keepdim=True)
    dS = rb(Pb * ((i.DO @ i.V.transpose(-1, -2)) * g - delta))
    Pbt = rb(Pb * g)
    sc = float(np.float32(SCALE))
    out = dict(o=unheads(o), lse2=lse2.squeeze(-1), dv=unheads(rb(Pbt.transpose(-1, -2) @ i.DO)),
               dq1=unheads(rb(sc * (dS @ i.K1))), dk1=unheads(rb(sc * (dS.transpose(-1, -2) @ i.Q1))))
    if parts == 2:
        out.update(dq2=unheads(rb(sc * (dS @ i.K2))), dk2=unheads(rb(sc * (dS.transpose(-1, -2) @ i.Q2))))
    return out


# ------------------------------------------------------------------------------------------------ the conditions
def round_trips(p):
    """Every operand is a bf16 (and, for the fp8 profiles, MX e4m3) value, and so is 0.125 q."""
    for t in (p.q1, p.k1, p.v, p.q2, p.k2, p.dout):
        if t is None:
            continue
        assert torch.equal(t, t.round()) and float(t.abs().max()) <= 256
        assert torch.equal(t.bfloat16().float(), t)
    for q in (p.q1, p.q2):
        if q is not None:
            assert torch.equal((q * 0.125).bfloat16().float(), q * 0.125)
    return True


def leave_one_out(p, i, keys):
    """Key j = keys[b,h,q,r] left out of query q, pass by pass as the kernels are built.  The forward loses it from the
    softmax: with p = P[q, j], o' = (o - g p v_j) / (1 - p).  The dq pass takes lse2 and delta from the forward, so what
    it loses is the key's term: dq' = dq - scale dS[q, j] k_j.  (The dk / dv pass loses the key's own rows.)
    -> |o' - o|, |dq1' - dq1|, |dq2' - dq2| or None, each [B,H,Tq,R,32]."""
    pj = i.P.gather(-1, keys)                                                         # [B,H,Tq,R]
    one_m = (i.P.sum(-1, keepdim=True) - pj).clamp_min(1e-300)
    gj = torch.ones_like(pj) if i.g is None else i.g.gather(-1, keys)
    at = lambda t: t.unsqueeze(2).expand(-1, -1, keys.shape[2], -1, -1).gather(3, keys.unsqueeze(-1).expand(-1, -1, -1, -1, 32))
    o1 = (i.o.unsqueeze(3) - (gj * pj).unsqueeze(-1) * at(i.V)) / one_m.unsqueeze(-1)
    dSj = i.dS.gather(-1, keys).abs().unsqueeze(-1)
    return [(o1 - i.o.unsqueeze(3)).abs()] + [None if K is None else NAT * dSj * at(K).abs() for K in (i.K1, i.K2)]


def class_members(shape, call, max_members=8):
    """keys[b,h,q,r]: the keys of query q's target class in the pointer layout (padded with the first), and a mask."""
    B, H, Tq, S, parts = shape
    lay = layout(shape)
    cls0 = _key_class(shape)
    u = (torch.arange(Tq) + (call // 2) * Tq) % lay.smod
    same = (cls0.view(1, S) % lay.smod == u.view(Tq, 1)) if parts == 1 else (cls0.view(1, S) == u.view(Tq, 1))
    order = torch.argsort((~same).int(), dim=-1, stable=True)[:, :max_members]        # members first
    mask = same.gather(-1, order)
    keys = torch.where(mask, order, order[:, :1])
    return keys.view(1, 1, Tq, -1).expand(B, H, Tq, -1).contiguous(), mask.view(1, 1, Tq, -1).expand(B, H, Tq, -1)


def pointer_detection(shape, profile, dtype="bf16", o_factor=None, detect=DETECT, detect_dq=None):
    """Over the calls of a pointer / dropout case: which keys a leave-one-out moves some element of o, dq1, dq2 (through
    the queries that target them) and of dk1, dk2, dv (their own rows vanish) by `detect` tolerances, and which query
    rows move some element of dv by as much when they are left out of the dk / dv sums.
    Under dropout a key is asked of o / dq only where a query that targets it keeps it, a row only where it keeps a key of
    its class (a dropped probability carries nothing).  -> ({pass: bool [B,H,S]}, rows bool [B,H,Tq], the same two for
    what is asked)"""
    B, H, Tq, S, parts = shape
    f = dict(FACTOR[dtype])
    if o_factor is not None:
        f["o"] = o_factor
    seen = {n: torch.zeros(B, H, S, dtype=torch.bool) for n in PASSES if parts == 2 or not n.endswith("2")}
    rows = torch.zeros(B, H, Tq, dtype=torch.bool)
    need = {n: torch.zeros(B, H, S, dtype=torch.bool) if n in ("o", "dq1", "dq2") else torch.ones(B, H, S, dtype=torch.bool) for n in seen}
    need_rows = torch.zeros(B, H, Tq, dtype=torch.bool)
    onto_keys = lambda hit: torch.zeros(B, H, S, dtype=torch.int32).scatter_add_(-1, keys.flatten(2), hit.flatten(2).int()) > 0
    for call in range(n_calls(shape, profile)):
        p = problem(shape, profile, call)
        i = with_internals(p)["_"]
        keys, mask = class_members(shape, call)
        kept = mask if i.g is None else mask & (i.g.gather(-1, keys) > 0)
        need_rows |= (kept & (i.DO.abs().sum(-1, keepdim=True) > 0)).any(-1)
        for name in ("o", "dq1", "dq2"):
            if name in need:
                need[name] |= onto_keys(kept)
        d_o, d_q1, d_q2 = leave_one_out(p, i, keys)
        hA = lambda name: heads(p.A[name], H)
        for name, delta in (("o", d_o), ("dq1", d_q1), ("dq2", d_q2)):
            if delta is None:
                continue
            times = detect if name == "o" or detect_dq is None else detect_dq
            hit = ((delta >= times * f[name] * hA(name).unsqueeze(3)) & (delta > 0)).any(-1) & mask       # [B,H,Tq,R]
            seen[name] |= onto_keys(hit)
        for name in ("dk1", "dv", "dk2"):
            if name in seen:
                own = heads(p.ref[name], H).abs()
                seen[name] |= ((own >= detect * f[name] * hA(name)) & (own > 0)).any(-1)
        # a query row left out of the dv sums: dv[s, c] loses Pd[q, s] dO[q, c], looked for at the keys of its class
        pd = i.Pd.gather(-1, keys) * mask                                                 # [B,H,Tq,R]
        a_dv = hA("dv").unsqueeze(2).expand(-1, -1, Tq, -1, -1).gather(3, keys.unsqueeze(-1).expand(-1, -1, -1, -1, 32))
        lost = pd.unsqueeze(-1) * i.DO.abs().unsqueeze(3)
        rows |= ((lost >= detect * f["dv"] * a_dv) & (lost > 0)).flatten(3).any(-1)
    return seen, rows, need, need_rows


def flat_detection(shape, dtype="bf16", o_factor=None, detect=DETECT):
    """The flat profile's unit is an aligned run of 32 keys (a ragged tail belongs to the last run): {pass: [runs] bool},
    True where leaving the run out of the pass (leave_one_out says how) moves some element by `detect` tolerances.  dk is
    exactly zero and is not fed; a run that holds every key cannot be left out."""
    B, H, Tq, S, parts = shape
    f = dict(FACTOR[dtype])
    if o_factor is not None:
        f["o"] = o_factor
    p = problem(shape, "flat", 0)
    names = ["o", "dq1", "dv"] + (["dq2"] if parts == 2 else [])
    starts = list(range(0, S - S % 32, 32)) or [0]
    runs = [(a, S if a == starts[-1] else a + 32) for a in starts]                 # a ragged tail belongs to the last run
    runs = [r for r in runs if r != (0, S)]
    seen = {n: torch.zeros(len(runs), dtype=torch.bool) for n in names}
    i = with_internals(p)["_"]
    for k, (a, b) in enumerate(runs):
        w = torch.ones(1, 1, 1, S, dtype=torch.float64)
        w[..., a:b] = 0.0
        change = dict(o=(attend64(p, w=w)["o"] - p.ref["o"]).abs())                  # the forward: out of the softmax
        change["dq1"] = unheads(NAT * (i.dS[..., a:b] @ i.K1[..., a:b, :])).abs()    # the dq pass: the run's terms
        if parts == 2:
            change["dq2"] = unheads(NAT * (i.dS[..., a:b] @ i.K2[..., a:b, :])).abs()
        own = torch.zeros_like(p.ref["dv"])
        own[:, a:b] = p.ref["dv"][:, a:b].abs()                                      # the dk / dv pass: the run's own rows
        change["dv"] = own
        for n in names:
            seen[n][k] = bool(((change[n] >= detect * f[n] * p.A[n]) & (change[n] > 0)).any())
    return seen


# ------------------------------------------------------------------------------------------------ the case list
EXACT_FAMILIES = ("attn_family", "attn_ksplit", "attn_strided", "attn_exact")


def runs():
    """[(case, profile)]: every attention case of the table on the pointer and the flat profile, the dropout cases on the
    dropout profile."""
    out, seen = [], set()
    for fam in EXACT_FAMILIES:
        for c in V.cases(fam, call="attn"):
            if V.case_id(c) in seen:                       # the same knobs, shape and dtype in two families: one run
                continue
            seen.add(V.case_id(c))
            if c.extra.get("drop"):
                out.append((c, "dropout"))
            else:
                out.extend([(c, "pointer"), (c, "flat")])
    return sorted(out, key=lambda cp: (cp[0].shape, cp[1], V.case_id(cp[0])))


def fp8_shapes():
    """The shapes that also run on the fp8 forward: FP8_SHAPES without the 1450 x 1450 one, plus the key-tile edges."""
    return [s for s in FP8_SHAPES if s[2:4] != (1450, 1450)] + [(1, 2, 77, s, 1 + s % 2) for s in (31, 32, 33, 64, 65)]


def run_id(c, profile):
    return f"{V.case_id(c)}-{profile}"


def shapes():
    """The distinct (shape, profile) pairs of runs()."""
    return sorted({(c.shape, prof) for c, prof in runs()})


def route_name(c):
    """fwd/dq/dkv family of a case, as the commit message lists them: e.g. lds8/lds/lds, split/split/prefetch-ks4-drop."""
    e = c.expect
    L = V.L
    fwd = "lds%d" % e["fwd_waves"] if e["fwd"] == L.ATTN_LDS else "split" if e["key_split"] else "plain"
    dq = "lds" if e["dq"] == L.ATTN_LDS else "split" if e["key_split"] else "plain"
    dkv = {L.ATTN_PLAIN: "plain", L.ATTN_LDS: "lds", L.ATTN_PREFETCH: "prefetch"}[e["dkv"]]
    return f"{c.dtype}:{fwd}/{dq}/{dkv}" + (f"-ks{e['ksplit']}" if e.get("ksplit", 1) > 1 else "") + ("-drop" if c.extra.get("drop") else "")
