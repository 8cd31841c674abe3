"""The selectable kernel variants and the smallest shapes that reach them: ONE table, read by tests/test_dispatch_cpu.py
(the route the library reports for every case, under the case's knobs, is held against the route written here -- no GPU
needed), by tests/test_variants_gpu.py (which runs every case against a high-precision torch reference) and, for the
attention cases, by tests/attention_cases.py (operands that leave the float64 reference exact).

A case records the knobs it sets (csrc/knobs.h), the call, the shape, the dtype and the route fields it expects.  Data
and small helpers only: no fixtures, nothing is computed on a device here."""
from collections import namedtuple

import torch

from future_od.native import lib as L
from future_od.native import ops

# family: which group of variants the case belongs to (the GPU tests select by it)
# knobs:  {FOD_X: value} in effect for the call
# call:   "gemm_nt" (M, N, K) | "gemm_tn" (M, N1, K2) | "conv_fwd" / "conv_dgrad" / "conv_wgrad" (Nimg, H, W, Cin, Cout, k,
#         stride, pad) | "attn" (B, H, Tq, S, parts) | "layernorm" (rows, D) | "attn_fp8" (B, H, Tq, S, parts)
# dtype:  "bf16" | "f32"
# expect: {route field: value}, every one compared with the library's answer (empty: the call has no route query)
# extra:  what else the call is made with (det: deterministic mode, drop: attention dropout, ...)
Case = namedtuple("Case", "family knobs call shape dtype expect extra")
DTYPE = {"bf16": torch.bfloat16, "f32": torch.float32}
CASES = []


def _add(family, knobs, call, shape, dtype, expect, **extra):
    CASES.append(Case(family, dict(knobs), call, tuple(shape), dtype, dict(expect), dict(extra)))


def cases(family, **where):
    """The cases of a family, optionally only those whose call / dtype / extra entries equal `where`."""
    out = []
    for c in CASES:
        if c.family != family:
            continue
        if all((getattr(c, k) if k in Case._fields else c.extra.get(k)) == v for k, v in where.items()):
            out.append(c)
    return out


def case_id(c):
    knobs = ",".join(f"{k[4:]}={v}" for k, v in c.knobs.items()) or "default"
    extra = "".join(f"-{k}{'' if v is True else v}" for k, v in c.extra.items() if v not in (False, None))
    return f"{c.call}-{'x'.join(map(str, c.shape))}-{c.dtype}-{knobs}{extra}"


def conv_geom(shape):
    n, h, w, cin, cout, k, stride, pad = shape
    return ops.conv_geom((n, h, w, cin), cout, k, stride, pad)


def route_of(c):
    """The library's route for the case's call under the knobs and the mode IN EFFECT (the caller sets them); None for a
    call without a route query."""
    dtype = DTYPE[c.dtype]
    if c.call == "gemm_nt":
        return ops.gemm_nt_route(*c.shape, dtype)
    if c.call == "gemm_tn":
        return ops.gemm_tn_route(*c.shape, dtype, row_scale=c.extra.get("row_scale", False), colsum=c.extra.get("colsum", False))
    if c.call in ("conv_fwd", "conv_dgrad", "conv_wgrad"):
        which = {"conv_fwd": L.CONV_FWD, "conv_dgrad": L.CONV_DGRAD, "conv_wgrad": L.CONV_WGRAD}[c.call]
        return ops.conv2d_route(which, conv_geom(c.shape), dtype)
    if c.call == "attn":
        B, H, Tq, S, parts = c.shape
        return ops.attn_route(B, H, Tq, S, parts, dtype, drop_p=c.extra.get("drop", 0.0))
    return None


def route_mismatches(c):
    """[(field, reported, expected)] of the case's route under its knobs and mode; the knobs and the mode are put back."""
    was = ops.is_deterministic()
    try:
        ops.set_deterministic(bool(c.extra.get("det", False)))
        with L.knobs(**c.knobs):
            r = route_of(c)
    finally:
        ops.set_deterministic(was)
    if r is None:
        return []
    return [(f, getattr(r, f), v) for f, v in c.expect.items() if getattr(r, f) != v]


def assert_route(c):
    """The call that follows takes the kernel the table says (ask with the case's knobs and mode already in effect)."""
    r = route_of(c)
    if r is not None:
        bad = [(f, getattr(r, f), v) for f, v in c.expect.items() if getattr(r, f) != v]
        assert not bad, (case_id(c), bad)
    return r


BOTH = ("bf16", "f32")

# ---- NT contractions and convolutions, 128-row kernel with the 128-wide tile (FOD_NT_NARROW=1: narrow tiles only for N <= 64)
NT128_KNOBS = dict(FOD_NT_NARROW=1, FOD_NT_SMALL=0)
NT128 = dict(kernel=L.NT_128, tile_n=128, stages=2, ksplit=1)
NT128_DENSE = [(300, 200, 64), (257, 132, 256), (1, 264, 16), (130, 72, 96),
               (150, 130, 64)]                       # N % 4 != 0: the scalar epilogue
NT128_EPILOGUE = (150, 200, 64)                      # the shape of test_gemm_nt_epilogue
NT128_CONV = [(3, 9, 11, 128, 72, 1, 1, 0), (1, 15, 21, 136, 136, 3, 2, 1), (2, 9, 12, 200, 72, 1, 2, 0),
              (2, 15, 20, 72, 200, 3, 1, 1)]
for _dt in BOTH:
    for _s in NT128_DENSE:
        _add("nt128", NT128_KNOBS, "gemm_nt", _s, _dt, NT128, epilogue="scalar" if _s[1] % 4 else "vector")
    _add("nt128", NT128_KNOBS, "gemm_nt", NT128_EPILOGUE, _dt, NT128, epilogue="vector", full_epilogue=True)
    for _s in NT128_CONV:
        _add("nt128", NT128_KNOBS, "conv_fwd", _s, _dt, NT128)
        _add("nt128", NT128_KNOBS, "conv_dgrad", _s, _dt, NT128, stride=_s[6])

# ---- short-launch NT kernel, K split across blocks: ksplit = min(256 // tiles, cap, K // 256), cap = 4 unless the knob says
NT_SPLITK_SHAPES = [(256, 256, 2048), (37, 40, 2056), (130, 200, 1024), (64, 64, 1536)]
for _knob in (None, 0, 2, 3, 8):
    for (_M, _N, _K) in NT_SPLITK_SHAPES:
        _tiles = -(-_M // 64) * -(-_N // 64)
        _ks = 1 if _knob == 0 else min(256 // _tiles, 4 if _knob is None else _knob, _K // 256)
        _add("nt_splitk", {} if _knob is None else dict(FOD_NT_SPLITK=_knob), "gemm_nt", (_M, _N, _K), "bf16",
             dict(kernel=L.NT_SMALL, tile_n=64, ksplit=_ks))

# ---- 256-row LDS-DMA kernel: interleaved DMA requests crossed with the ring depth (3 stages: 256 x 128, 2: 256 x 256)
NT_BIG_KNOBS = dict(FOD_NT_BIG=2, FOD_NT_SMALL=0)
NT_BIG_3_0 = (dict(NT_BIG_KNOBS, FOD_NT_BIG_ILV=0), dict(kernel=L.NT_BIG, tile_n=128, stages=3, interleave=0))
NT_BIG_2_1 = (dict(NT_BIG_KNOBS, FOD_NT_BIG256=2, FOD_NT_BIG_ILV=1), dict(kernel=L.NT_BIG, tile_n=256, stages=2, interleave=1))
NT_BIG_3_1 = (NT_BIG_KNOBS, dict(kernel=L.NT_BIG, tile_n=128, stages=3, interleave=1))                       # the defaults
NT_BIG_2_0 = (dict(NT_BIG_KNOBS, FOD_NT_BIG256=2), dict(kernel=L.NT_BIG, tile_n=256, stages=2, interleave=0))
NT_BIG_DENSE = [(300, 256, 128), (257, 512, 256), (1000, 264, 72)]
NT_BIG_CONV_128 = [(2, 15, 20, 64, 64, 3, 1, 1), (1, 15, 21, 64, 128, 3, 2, 1)]        # two of BIG_CONV_CASES
NT_BIG_CONV_256 = [(2, 9, 12, 256, 512, 1, 2, 0), (2, 11, 13, 256, 320, 1, 1, 0)]      # two of BIG256_CONV_CASES
for _kn, _ex in (NT_BIG_3_0, NT_BIG_2_1):
    for _s in NT_BIG_DENSE:
        _add("nt_big", _kn, "gemm_nt", _s, "bf16", _ex)
for _kn, _ex in (NT_BIG_3_1, NT_BIG_2_0):
    _add("nt_big", _kn, "gemm_nt", NT_BIG_DENSE[0], "bf16", _ex)
for _s in NT_BIG_CONV_128 + NT_BIG_CONV_256:
    for _call in ("conv_fwd", "conv_dgrad"):
        _add("nt_big", NT_BIG_3_0[0], _call, _s, "bf16", NT_BIG_3_0[1])
for _s in NT_BIG_CONV_256:
    for _call in ("conv_fwd", "conv_dgrad"):
        _add("nt_big", NT_BIG_2_1[0], _call, _s, "bf16", NT_BIG_2_1[1])

# ---- TN 128 x 128 kernel: XCD-grouped order with a split count that is no multiple of 8 (the grid is rounded up to whole
# groups of 8 and the tail blocks return), the plain order, forced rows per split
TN128 = dict(kernel=L.TN_128, bi=128, bj=128, uses_partials_ws=0)
TN_OPERANDS = dict(row_scale=True, colsum=True)
for _dt in BOTH:
    _add("tn128", {}, "gemm_tn", (12300, 136, 72), _dt, dict(TN128, xcd_order=1, nsplit=23), **TN_OPERANDS)
    _add("tn128", {}, "gemm_tn", (12300, 136, 72), _dt, dict(TN128, xcd_order=1, nsplit=23, uses_partials_ws=1), det=True,
         **TN_OPERANDS)
    _add("tn128", {}, "gemm_tn", (4100, 264, 136), _dt, dict(TN128, xcd_order=1, nsplit=8), **TN_OPERANDS)
    _add("tn128", dict(FOD_TN_XCD=0), "gemm_tn", (4100, 264, 136), _dt, dict(TN128, xcd_order=0, nsplit=8), **TN_OPERANDS)
    _add("tn128", dict(FOD_TN_ROWS=256), "gemm_tn", (4100, 264, 136), _dt, dict(TN128, xcd_order=1, nsplit=15), **TN_OPERANDS)
    _add("tn128", dict(FOD_TN_ROWS=520), "gemm_tn", (4700, 264, 136), _dt, dict(TN128, xcd_order=0, nsplit=10), **TN_OPERANDS)

# ---- TN 8-wave kernel from 8192 rows on: partial tiles in the caller's workspace and the reduce launch, ragged N1 / K2
TN_BIG_KNOBS = dict(FOD_TN_BIG=2, FOD_TN_SMALL=0)
TN_BIG_SHAPES = [(8200, 136, 72), (8200, 264, 392)]
TN_BIG_CONV = (1, 82, 100, 72, 136, 3, 1, 1)          # 8200 output pixels, dW [136, 3 * 3 * 72]
for _ws in (1, 0):
    _kn = dict(TN_BIG_KNOBS) if _ws else dict(TN_BIG_KNOBS, FOD_TN_WS=0)
    for _s in TN_BIG_SHAPES:
        _add("tn_big", _kn, "gemm_tn", _s, "bf16", dict(kernel=L.TN_BIG, uses_partials_ws=_ws, nsplit=26, xcd_order=1),
             **TN_OPERANDS)
    _add("tn_big", _kn, "conv_wgrad", TN_BIG_CONV, "bf16", dict(kernel=L.TN_BIG, uses_partials_ws=_ws, nsplit=26, xcd_order=1),
         row_scale=True)
_add("tn_big", dict(TN_BIG_KNOBS, FOD_TN_BIG256=2), "gemm_tn", TN_BIG_SHAPES[1], "bf16",
     dict(kernel=L.TN_BIG, bi=256, bj=256, uses_partials_ws=1, nsplit=26), **TN_OPERANDS)
_add("tn_big", TN_BIG_KNOBS, "gemm_tn", TN_BIG_SHAPES[0], "bf16", dict(kernel=L.TN_BIG, uses_partials_ws=1, nsplit=26), det=True,
     **TN_OPERANDS)

# ---- layer norm: every instantiated width, around the many-row threshold (rows >= 8192: 16 or 8 lanes per row); the row
# groups a wave of the many-row backward walks (FOD_LN_BWD_GROUPS) have no route query: the knob is only read back
LN_WIDTHS = (64, 128, 192, 256, 320, 384, 448, 512)
LN_ROWS = (37, 8191, 8192, 8200)
LN_GROUPS = (1, 4, 16)
for _dt in BOTH:
    for _D in LN_WIDTHS:
        for _rows in LN_ROWS:
            for _g in (LN_GROUPS if _rows >= 8192 else (None,)):
                _add("layernorm", {} if _g is None else dict(FOD_LN_BWD_GROUPS=_g), "layernorm", (_rows, _D), _dt, {})

# ---- attention families (bf16).  Shapes with Tq > 512 or S < 128 are the LDS kernels' by default, the others the
# in-block key split's; what each knob set turns them into:
PLAIN, LDS, PREFETCH = L.ATTN_PLAIN, L.ATTN_LDS, L.ATTN_PREFETCH


def _fam(fwd, dq, dkv, waves, key_split, ksplit=1):
    return dict(fwd=fwd, dq=dq, dkv=dkv, fwd_waves=waves, key_split=key_split, ksplit=ksplit)


ATTN_LONG_SHAPES = [(1, 2, 600, 333, 1), (2, 1, 513, 64, 2), (1, 8, 128, 49, 2), (2, 2, 33, 1, 2), (1, 2, 700, 650, 2)]
ATTN_LONG_KNOB_SETS = [
    (dict(FOD_ATTN_LDS=0), _fam(PLAIN, PLAIN, PREFETCH, 4, 0)),
    (dict(FOD_ATTN_LDS=4), _fam(LDS, LDS, LDS, 4, 0)),
    (dict(FOD_ATTN_PF=0), _fam(LDS, LDS, LDS, 8, 0)),                 # the LDS trio does not look at FOD_ATTN_PF
    (dict(FOD_ATTN_LDS=0, FOD_ATTN_PF=0), _fam(PLAIN, PLAIN, PLAIN, 4, 0)),
    (dict(FOD_ATTN_LDS=4, FOD_ATTN_PF=0), _fam(LDS, LDS, LDS, 4, 0)),
]
for _kn, _ex in ATTN_LONG_KNOB_SETS:
    for _s in ATTN_LONG_SHAPES:
        _add("attn_family", _kn, "attn", _s, "bf16", _ex)
_add("attn_family", {}, "attn", ATTN_LONG_SHAPES[0], "bf16", _fam(LDS, LDS, LDS, 8, 0))
ATTN_SPLIT_SHAPES = [(1, 1, 40, 130, 2), (2, 4, 77, 150, 1)]          # S < 256: split inside the block only
for _s in ATTN_SPLIT_SHAPES:
    _add("attn_family", dict(FOD_ATTN_PF=0), "attn", _s, "bf16", _fam(PLAIN, PLAIN, PLAIN, 4, 1))
    _add("attn_family", {}, "attn", _s, "bf16", _fam(PLAIN, PLAIN, PREFETCH, 4, 1))
# dropout never takes the LDS kernels; with FOD_ATTN_PF=0 its dK/dV pass is the plain kernel
_add("attn_family", dict(FOD_ATTN_PF=0), "attn", (1, 2, 600, 333, 1), "bf16", _fam(PLAIN, PLAIN, PLAIN, 4, 0), drop=0.1)
_add("attn_family", dict(FOD_ATTN_PF=0), "attn", (2, 4, 77, 150, 1), "bf16", _fam(PLAIN, PLAIN, PLAIN, 4, 1), drop=0.1)
# the rare branches of the LDS forwards (forced rescales, saturated softmax), four and eight waves
ATTN_EXTREME_SHAPE = (1, 2, 600, 460)
ATTN_SATURATED_SHAPE = (1, 2, 600, 200, 1)
for _kn, _waves in ((dict(FOD_ATTN_LDS=4), 4), ({}, 8)):
    for _parts in (1, 2):
        _add("attn_extreme", _kn, "attn", ATTN_EXTREME_SHAPE + (_parts,), "bf16", _fam(LDS, LDS, LDS, _waves, 0))
_add("attn_saturated", dict(FOD_ATTN_LDS=4), "attn", ATTN_SATURATED_SHAPE, "bf16", _fam(LDS, LDS, LDS, 4, 0))

# ---- attention, keys split across blocks (Tq <= 512, S >= 256, the caller's scratch): (shape, ksplit, kchunk)
ATTN_KSPLIT = [((1, 1, 33, 2000, 2), 8, 256),        # last chunk 208 keys
               ((1, 2, 512, 700, 2), 3, 256),        # Tq at the boundary
               ((1, 4, 200, 300, 1), 2, 256),        # last chunk 44 keys
               ((1, 1, 64, 256, 1), 2, 128),
               ((1, 8, 256, 512, 1), 4, 128),
               ((1, 1, 64, 255, 1), 1, 255)]         # one key short: no split
for _dt in BOTH:
    for _s, _ks, _kc in ATTN_KSPLIT:
        _add("attn_ksplit", {}, "attn", _s, _dt,
             dict(_fam(PLAIN, PLAIN, PREFETCH if _dt == "bf16" else PLAIN, 4, 1, _ks), kchunk=_kc))

# ---- attention on strided operands (Tq = S: q / k / v column slices of one buffer, a batch-shared k2 table, gradient slots
# inside larger buffers): once per family
_add("attn_strided", {}, "attn", (2, 2, 100, 100, 2), "bf16", _fam(LDS, LDS, LDS, 8, 0))
_add("attn_strided", {}, "attn", (2, 2, 300, 300, 2), "bf16", dict(_fam(PLAIN, PLAIN, PREFETCH, 4, 1, 2), kchunk=256))
_add("attn_strided", dict(FOD_ATTN_LDS=0), "attn", (2, 2, 100, 100, 2), "bf16", _fam(PLAIN, PLAIN, PREFETCH, 4, 0))

# ---- attention on exactly representable operands (tests/attention_cases.py runs these together with every attn_family /
# attn_ksplit / attn_strided case): the default routes of both dtypes at the shapes of test_attention_fwd_bwd, f32 where
# the families above have bf16 only, dropout by default and with FOD_ATTN_PF=0, and the smallest shapes on the kernels'
# edges.  The expected route restates route() of csrc/attention.hip for the default knobs (FOD_ATTN_LDS=8).
def _attn_default(shape, dtype, drop=False, pf=True):
    B, H, Tq, S, _ = shape
    split = int(Tq <= 512 and S >= 128)
    lds = dtype == "bf16" and not drop and not split
    ks, kc = 1, S
    if Tq <= 512 and S >= 256:
        k = min(256 // (-(-Tq // 32) * H * B), 8, S // 128)
        if k > 1:
            kc = -(-(-(-S // k)) // 128) * 128
            ks = -(-S // kc)
    fwd = LDS if lds else PLAIN
    dkv = LDS if lds else PREFETCH if dtype == "bf16" and pf else PLAIN
    return dict(_fam(fwd, fwd, dkv, 8 if lds else 4, split, ks), kchunk=kc)


ATTN_FWD_BWD_SHAPES = [(2, 4, 77, 150, 1), (1, 8, 128, 49, 2), (2, 2, 33, 1, 2), (1, 8, 200, 200, 1), (2, 8, 128, 1450, 2),
                       (1, 2, 600, 333, 1), (1, 1, 40, 130, 2), (1, 2, 700, 650, 2), (2, 1, 513, 64, 1)]
ATTN_EDGE_TQ = (32, 33, 128, 129, 256, 257)          # one wave's queries, a 4-wave and an 8-wave block, each plus one
ATTN_EDGE_S = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)   # key tiles of 32 / 64, the two split thresholds
ATTN_EDGE_SHAPES = ([(1, 2, _tq, _s, 1 + (_tq + _s) % 2) for _tq in ATTN_EDGE_TQ for _s in (65, 129)]       # S = 129: S % 128 == 1
                    + [(1, 2, 33, _s, 1 + _s % 2) for _s in ATTN_EDGE_S if _s not in (65, 129)]
                    + [(1, 1, 513, _s, 1 + _s % 2) for _s in ATTN_EDGE_S if _s != 1])      # the non-split kernels at every S
ATTN_DROP_SHAPES = [(1, 2, 600, 333, 1), (2, 4, 77, 150, 1), (1, 4, 200, 300, 1), (1, 8, 128, 49, 2)]
_seen = set()
for _dt in BOTH:
    for _s in ATTN_FWD_BWD_SHAPES + ATTN_LONG_SHAPES + ATTN_SPLIT_SHAPES + ATTN_EDGE_SHAPES:
        if (_s, _dt) not in _seen:
            _seen.add((_s, _dt))
            _add("attn_exact", {}, "attn", _s, _dt, _attn_default(_s, _dt))
    for _s in ATTN_DROP_SHAPES:
        _add("attn_exact", {}, "attn", _s, _dt, _attn_default(_s, _dt, drop=True), drop=0.5)
        _add("attn_exact", dict(FOD_ATTN_PF=0), "attn", _s, _dt, _attn_default(_s, _dt, drop=True, pf=False), drop=0.5)

# ---- fp8 attention forward with two 64-key tiles per barrier (no route query: the knob is only read back)
FP8_STAGE2_SHAPES = [(1, 2, 77, 150, 1), (2, 2, 33, 1, 2), (1, 1, 300, 64, 2), (1, 2, 600, 333, 1)]
for _s in FP8_STAGE2_SHAPES:
    for _peaked in (False, True):
        _add("fp8_stage2", dict(FOD_FP8_STAGE=2), "attn_fp8", _s, "bf16", {}, peaked=_peaked)
