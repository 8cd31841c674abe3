"""Operands for which the FUSED kernels' arithmetic is exact, their float64 references and the table of cases: the frozen
bottleneck in one launch (csrc/bottleneck_fused.hip, both kernels, both shortcut forms) and the forward of the fused
projection + add + norm (csrc/linear_norm.hip).  The sibling of tests/exact_cases.py, read by tests/test_exact_cases_cpu.py
(preconditions, census, clamp caps, mutants of the reference -- no GPU) and by tests/test_exact_gpu.py (torch.equal).

The bottleneck chains three contractions and rounds the two 64-channel intermediates to bf16 in between, so equality needs
every stored intermediate to BE a bf16 number before its rounding, every f32 partial sum an exact dyadic below 2^24 units,
and every value before the final rounding at most 256 in magnitude (the convention of exact_cases.pm1).  A dense 576-term
contraction of 8-bit values cannot have that at all three stages at once; so there are three operand PROFILES, each with one
stage dense in non-zero +-1 operands and the two others thin: one tap of +1 (or +-1/2) per output channel, a signed gather
that hands the dense stage's result on unchanged and exercises the tap and border addressing.

  s1  conv1 dense:   x +-1, W1 +-1, b1 = 32 (Cin 64) or 64 (Cin 256) + {-2..2};  W2 one +1 tap per output channel (all nine
                     tap positions, the input channels a permutation), b2 {-2..2};  W3 one +1 tap, b3 {0..4}
  s2  3x3 dense:     W1 one +-1/2 tap per output channel, b1 = 1.5 (Y1 is 1 or 2, never 0: padding applied to x instead of Y1
                     would put relu(b1) = 1.5 on the halo);  W2 +-1 on all 576 taps, b2 = 64 + {-2..2};  W3 thin as in s1
  s3  expansion and shortcut dense:  W1 thin as in s2;  W2 thin as in s1 but b2 in {1, 2}, so that Y2 -- the dense stage's
                     operand -- is 1..4 and never 0, on the border too;  W3 +-1, b3 = 48 + {-2..2}
In every profile the projection shortcut (Cin 64) is a dense +-1 wd with bd in {-2..2}; the identity shortcut is x itself.

The reference is float64 torch on the CPU with ResNet bottleneck semantics (Y1 = relu(conv1x1(x) + b1), zero outside the image;
Y2 = relu(conv3x3(Y1, pad 1) + b2); out = relu(conv1x1(Y2) + b3 + shortcut)), rounded ONCE to bf16 at the end.  Data and
small helpers only: nothing is computed on a device here."""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

import exact_cases as E

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
TH, TW = 6, 30                         # the output tile of both kernels (csrc/bottleneck_fused.hip); halos are 8 x 32
PROFILES = ("s1", "s2", "s3")
DENSE_STAGE = {"s1": 1, "s2": 2, "s3": 3}
CINS = (64, 256)                       # 64: projection shortcut, 256: identity

# (N, H, W) -> what the shape is in the table for
SHAPES = {
    (1, 1, 1): "sub-tile", (3, 1, 1): "sub-tile", (2, 3, 5): "sub-tile", (1, 13, 2): "sub-tile", (1, 2, 33): "sub-tile",
    # ^ smaller than a tile or a halo row; several single-pixel images: a workgroup's tile range crosses image boundaries
    (1, 6, 30): "one-tile", (1, 5, 29): "one-tile", (1, 7, 31): "one-tile",
    # ^ exactly one tile, one short in both directions, one over in both (4 tiles, three of them one pixel wide or high:
    #   the stores of a partial tile)
    (1, 12, 60): "seams",              # 2 x 2 full tiles: every interior seam and the four-tile corner
    (2, 23, 41): "ragged",             # the shape of test_fused_frozen_bottleneck_matches_the_layer_by_layer_path
    # more tiles than compute units (256 on the MI355X): 270 tiles -> two per workgroup, 135 of the 256 workgroups have
    # work; 665 tiles (7 x 19 per image) -> three per workgroup, ranges that start mid-image, the last one 2 tiles long.
    # The smallest shapes at which the ring wraps around, chunks are requested across tile boundaries and the tail is
    # issued out of range.
    (3, 36, 450): "walk-2", (5, 37, 570): "walk-3",
}
WALK = {"walk-2": dict(per=2, short_last=False), "walk-3": dict(per=3, short_last=True)}
V2_SHAPES = [s for s, why in SHAPES.items() if why in ("sub-tile", "one-tile", "ragged")]         # the edges and one multi-tile shape
BIG = 20000                            # pixels from which a problem is not kept after its next use (memory)


def ntiles(shape):
    n, h, w = shape
    return n * -(-h // TH) * -(-w // TW)


def walk_of(shape, cus):
    """What the persistent kernel does with the shape on a device of `cus` compute units: (workgroups launched, tiles per
    workgroup, workgroups with work, length of the last range, whether a range starts inside an image)."""
    t = ntiles(shape)
    grid = min(t, cus)
    per = -(-t // grid)
    busy = -(-t // per)
    per_image = t // shape[0]
    return dict(grid=grid, per=per, busy=busy, last=t - (busy - 1) * per, mid_image=any((i * per) % per_image for i in range(busy)))


# ------------------------------------------------------------------------------------------------ operands
def _perm(n, seed):
    return torch.randperm(n, generator=E._gen(seed))


def thin_w1(cin, seed):
    """[64, Cin]: one +-1/2 per output channel, on 64 different input channels that reach every 64-channel group of x."""
    src = _perm(cin, seed)[:64] if cin == 64 else (64 * (torch.arange(64) % (cin // 64)) + _perm(64, seed))[_perm(64, seed + 1)]
    w = torch.zeros(64, cin)
    w[torch.arange(64), src] = E.pick((64,), seed + 2, (-0.5, 0.5))
    return w


def thin_w2(seed):
    """[64, 3, 3, 64]: one +1 per output channel; every one of the nine tap positions is used, the input channels are a
    permutation (every Y1 channel is read)."""
    tap = (torch.arange(64) % 9)[_perm(64, seed)]
    w = torch.zeros(64, 3, 3, 64)
    w[torch.arange(64), tap // 3, tap % 3, _perm(64, seed + 1)] = 1.0
    return w


def thin_w3(seed):
    """[256, 64]: one +1 per output channel; every Y2 channel is read four times."""
    w = torch.zeros(256, 64)
    w[torch.arange(256), (torch.arange(256) % 64)[_perm(256, seed)]] = 1.0
    return w


def operands(profile, cin, shape, seed=1):
    """The bottleneck's operands on the CPU in the dtypes ops.bottleneck_fused_fwd takes: x NHWC bf16, weights bf16 in the
    layout prep_conv produces ([Cout][kh][kw][Cin]), shifts f32; wd / bd None for the identity block."""
    n, h, w = shape
    s = seed * 1000 + cin + 10 * PROFILES.index(profile)
    o = dict(x=E.pm1((n, h, w, cin), s + 1))
    if profile == "s1":
        o.update(w1=E.pm1((64, cin), s + 2), b1=(32.0 if cin == 64 else 64.0) + E.ints((64,), s + 3, -2, 2))
    else:
        o.update(w1=thin_w1(cin, s + 2), b1=torch.full((64,), 1.5))
    if profile == "s2":
        o.update(w2=E.pm1((64, 3, 3, 64), s + 10), b2=64.0 + E.ints((64,), s + 11, -2, 2))
    else:
        o.update(w2=thin_w2(s + 10), b2=E.ints((64,), s + 12, -2, 2) if profile == "s1" else E.ints((64,), s + 12, 1, 2))
    if profile == "s3":
        o.update(w3=E.pm1((256, 64), s + 20), b3=48.0 + E.ints((256,), s + 21, -2, 2))
    else:
        o.update(w3=thin_w3(s + 20), b3=E.ints((256,), s + 22, 0, 4))
    o.update(wd=E.pm1((256, 64), s + 30), bd=E.ints((256,), s + 31, -2, 2)) if cin == 64 else o.update(wd=None, bd=None)
    for k in ("x", "w1", "w2", "w3", "wd"):
        if o[k] is not None:
            assert torch.equal(o[k].to(BF16).float(), o[k]), k
            o[k] = o[k].to(BF16).contiguous()
    return o


# ------------------------------------------------------------------------------------------------ the reference
Stages = namedtuple("Stages", "y1 y2 pre y1_pre y2_pre")        # NHWC; *_pre / pre: before the relu


def forward(o, mutant=None, dtype=F64, store=lambda t: t):
    """The block in `dtype` arithmetic; `store` is applied to Y1 and Y2 (the identity here: for the table's operands they are
    bf16 numbers already; a rounding to bf16 for operands that are not).  `mutant`: (name, ...), a defect put into the
    computation on purpose (mutants() below; tests/test_exact_cases_cpu.py: each one must change the expected output)."""
    kind = mutant[0] if mutant else None
    x = o["x"].to(dtype)
    n, h, w, cin = x.shape
    w1, w2, w3 = o["w1"].to(dtype), o["w2"].to(dtype), o["w3"].to(dtype)
    b1, b2, b3 = o["b1"].to(dtype), o["b2"].to(dtype), o["b3"].to(dtype)
    y1_pre = x @ w1.t() + b1
    if kind in ("lose_product", "double_product") and mutant[1] == 1:
        (i, y, xx, c, k) = mutant[2]
        y1_pre[i, y, xx, c] += (1 if kind == "double_product" else -1) * w1[c, k] * x[i, y, xx, k]
    y1 = store(y1_pre.clamp(min=0))
    y1p = F.pad(y1, (0, 0, 1, 1, 1, 1))                      # the 3x3's zero padding applies to conv1's OUTPUT
    if kind == "pad_x":                                      # ... not to x: the halo would hold relu(b1)
        y1p = store((F.pad(x, (0, 0, 1, 1, 1, 1)) @ w1.t() + b1).clamp(min=0))
    if kind == "wrong_image":                                # the halo row above image i read from image i - 1's last row
        i = mutant[1]
        y1p[i, 0, 1:-1] = y1[i - 1, h - 1]
    y2_pre = b2.expand(n, h, w, 64).clone()
    for ky in range(3):
        for kx in range(3):
            y2_pre += y1p[:, ky:ky + h, kx:kx + w] @ w2[:, ky, kx].t()
    if kind in ("lose_product", "double_product") and mutant[1] == 2:
        (i, y, xx, c, ky, kx, k) = mutant[2]
        y2_pre[i, y, xx, c] += (1 if kind == "double_product" else -1) * w2[c, ky, kx, k] * y1p[i, y + ky, xx + kx, k]
    y2 = store(y2_pre.clamp(min=0))
    if kind == "seam":                                       # the last column of tile (0, 0)'s Y2 taken from the tile to its right
        y2[0, :TH, TW - 1] = y2[0, :TH, TW]
    if kind == "row_copy":                                   # one row of tile (0, 0) copied from the row below it, in one channel
        y2[0, mutant[1], :TW, mutant[2]] = y2[0, mutant[1] + 1, :TW, mutant[2]]
    pre = y2 @ w3.t() + b3
    if kind in ("lose_product", "double_product") and mutant[1] == 3:
        (i, y, xx, c, k) = mutant[2]
        pre[i, y, xx, c] += (1 if kind == "double_product" else -1) * w3[c, k] * y2[i, y, xx, k]
    if o["wd"] is None:
        pre += x
    else:
        pre += x @ o["wd"].to(dtype).t()
        if kind != "no_bd":
            pre += o["bd"].to(dtype)
    return Stages(y1, y2, pre, y1_pre, y2_pre)


def rounded(st):
    """The ONE rounding: relu, then bf16."""
    return st.pre.clamp(min=0).to(F32).to(BF16)


Problem = namedtuple("Problem", "ops want facts stats")


def _bf16_number(t):
    return bool(torch.equal(t.to(F32).to(BF16).to(t.dtype), t))


def _problem(profile, cin, shape, seed):
    """The operands, the expected output and the facts that make equality the right comparison:
    (a) every operand of the dense stage (and of the projection shortcut) is non-zero;
    (b) the sum of magnitudes of every stage's terms is below 2^24 units of the smallest step in play (1/2): every partial
        sum in an f32 accumulator is exact in any order;
    (c) Y1 and Y2 are bf16 numbers before their rounding -- the reference has no intermediate rounding to disagree about;
    (d) |value before the relu and the final rounding| + 1 <= 256: it and both integer neighbours are bf16 numbers;
    (e) where W2 is thin every Y1 channel is read by some tap, and every tap position is used.
    float64 throughout: the largest problem of the table takes about a second."""
    n, h, w = shape
    o = operands(profile, cin, shape, seed)
    st = forward(o)
    dense = DENSE_STAGE[profile]
    dense_ops = {1: (o["x"], o["w1"]), 2: (st.y1, o["w2"]), 3: (st.y2, o["w3"])}[dense] + (() if cin == 256 else (o["x"], o["wd"]))
    m = lambda t: float(t.abs().max())
    bounds = [cin * m(o["x"]) * m(o["w1"]) + m(o["b1"]), 576 * m(st.y1) * m(o["w2"]) + m(o["b2"]),
              64 * m(st.y2) * m(o["w3"]) + m(o["b3"]) + (m(o["x"]) if cin == 256 else 64 * m(o["x"]) * m(o["wd"]) + m(o["bd"]))]
    w2 = o["w2"].float()
    facts = {"a_dense_nonzero": all(bool((t != 0).all()) for t in dense_ops),
             "b_below_2^24": all(2 * b < E.TWO24 for b in bounds),
             "c_intermediates_are_bf16": _bf16_number(st.y1) and _bf16_number(st.y2),
             "d_bf16_integers": m(st.pre) + 1 <= 256 and bool((st.pre == st.pre.round()).all()),
             "e_thin_taps_reach_everything": profile == "s2" or (bool((w2.abs().sum((0, 1, 2)) > 0).all())
                                                                 and bool((w2.abs().sum((0, 3)) > 0).all()))}
    dense_out = {1: st.y1_pre, 2: st.y2_pre, 3: st.pre}[dense]
    stats = dict(max_y1=m(st.y1), max_y2=m(st.y2), max_pre=m(st.pre), dense_clamped=int((dense_out <= 0).sum()), dense_numel=dense_out.numel(),
                 out_clamped=int((st.pre <= 0).sum()), out_numel=st.pre.numel(), pixels=n * h * w)
    FACTS[(profile, cin, shape, seed)] = (facts, stats)
    return Problem(o, rounded(st), facts, stats)


FACTS = {}                                                   # the facts and the counts outlive a large problem's tensors
_small = functools.lru_cache(maxsize=None)(_problem)
_big = functools.lru_cache(maxsize=1)(_problem)              # 100 MB each: the table's cases of one shape follow each other


def problem(profile, cin, shape, seed=1):
    """Computed once per (profile, Cin, shape) and shared by the kernel versions and the tests; nobody writes to it."""
    n, h, w = shape
    return (_big if n * h * w >= BIG else _small)(profile, cin, tuple(shape), seed)


def facts_and_stats(profile, cin, shape, seed=1):
    key = (profile, cin, tuple(shape), seed)
    if key not in FACTS:
        problem(*key)
    return FACTS[key]


# ------------------------------------------------------------------------------------------------ mutants of the reference
def dense_product(profile, o, shape):
    """One product of the profile's dense stage that the thin stages behind it hand on, at the middle pixel of the last image:
    (stage, index).  s1: a Y1 channel that a CENTRE tap of the thin W2 reads (the others are read from a neighbouring pixel,
    which a one-pixel image does not have); s2: the centre tap."""
    n, h, w = shape
    stage, px = DENSE_STAGE[profile], (n - 1, h // 2, w // 2)
    if stage == 1:
        return stage, px + (int(o["w2"].float()[:, 1, 1].sum(0).argmax()), o["x"].shape[-1] - 1)
    return stage, px + ((63, 1, 1, 63) if stage == 2 else (255, 63))


def mutants(profile, cin, shape):
    """The defects that apply to the case: name -> the argument of forward()."""
    n, h, w = shape
    stage, where = dense_product(profile, problem(profile, cin, shape).ops, shape)
    out = {"lose_product": ("lose_product", stage, where), "double_product": ("double_product", stage, where)}
    if profile != "s1":
        out["pad_x"] = ("pad_x",)
    if w > TW:
        out["seam"] = ("seam",)
    if cin == 64:
        out["no_bd"] = ("no_bd",)
    if n > 1 and ntiles(shape) == n:                        # single-tile images: one workgroup's range crosses images
        out["wrong_image"] = ("wrong_image", 1)
    return out


# ------------------------------------------------------------------------------------------------ the tables
Bnk = namedtuple("Bnk", "profile cin version shape purpose seed")
# Seeds other than 1: the case's operands failed a precondition or a clamp cap with seed 1 (never a relaxed fact).
SEEDS = {}
BNK_CASES = [Bnk(p, cin, v, s, SHAPES[s], SEEDS.get((p, cin, s), 1))
             for p in PROFILES for cin in CINS for v in ("4", "2") for s in (SHAPES if v == "4" else V2_SHAPES)]


def bnk_id(c):
    return f"bnk-{c.profile}-cin{c.cin}-v{c.version}-{'x'.join(map(str, c.shape))}"


def bnk_params(**where):
    cs = [c for c in BNK_CASES if all(getattr(c, k) == v for k, v in where.items())]
    return dict(argvalues=cs, ids=[bnk_id(c) for c in cs])


def bnk_problem(c):
    return problem(c.profile, c.cin, c.shape, c.seed)


# ---- fod_linear_add_norm_fwd: sixteen rows per workgroup (M = 1, 15, 16, 17: ragged first and last groups; 100: seven groups)
Lan = namedtuple("Lan", "M bias then")
LAN_CASES = [Lan(M, b, t) for M in (1, 15, 16, 17, 100) for b in (True, False) for t in (False, True)]
# (A row-strided `a`, lda > 256, is not in the table: ops.linear_add_norm_fwd takes contiguous operands and passes lda = K.)


def lan_id(c):
    return f"lan-M{c.M}-{'bias' if c.bias else 'nobias'}-{'then' if c.then else 'plain'}"


def lan_params():
    return dict(argvalues=LAN_CASES, ids=[lan_id(c) for c in LAN_CASES])


LanProblem = namedtuple("LanProblem", "ops proj sum want_sum want_mean")


@functools.lru_cache(maxsize=None)
def lan_problem(M, bias):
    """a, w +-1, bias and x integers in -2..2: the projection a w^T + bias (which the kernel rounds to bf16 before it adds x, as
    the two launches it replaces do) and the sum are integers; the row mean is (a sum of 256 integers) * 2^-8, an exact f32
    number.  gamma, beta and the THEN form's weights are Gaussian: what depends on them is held to the toleranced bounds."""
    s = 7000 + M
    a, w, x = E.pm1((M, 256), s + 1).to(BF16), E.pm1((256, 256), s + 2).to(BF16), E.ints((M, 256), s + 3, -2, 2).to(BF16)
    b = E.ints((256,), s + 4, -2, 2) if bias else None
    g = torch.Generator().manual_seed(s + 5)
    gamma, beta = torch.rand(256, generator=g) + 0.5, torch.randn(256, generator=g) * 0.2
    then_w, then_b = (torch.randn(256, 256, generator=g) / 16).to(BF16), torch.randn(256, generator=g) * 0.3
    proj = a.double() @ w.double().t() + (b.double() if bias else 0)
    total = proj + x.double()
    mean = total.mean(-1)
    return LanProblem(dict(a=a, w=w, x=x, bias=b, gamma=gamma, beta=beta, then_w=then_w, then_b=then_b), proj, total,
                      total.to(F32).to(BF16), mean.to(F32))
