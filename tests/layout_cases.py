"""The copy, element-wise, layout, pooling and column-sum kernels of csrc/elementwise.hip, branch by branch: ONE table,
read by tests/test_permute_plan_cpu.py (a Python statement of every kernel's path conditions is applied to each case and
held against the path written here; a census counts the cases per path -- no GPU needed) and by tests/test_layout_gpu.py
(which runs every case against a plain CPU computation of the same operation).

Data and small helpers only: no fixtures, nothing is computed on a device here."""
import itertools
import zlib
from collections import namedtuple

import torch

DTYPE = {"bf16": torch.bfloat16, "f32": torch.float32}
ESIZE = {"bf16": 2, "f32": 4}
VEC = {"bf16": 8, "f32": 4}                     # elements per 16-byte access (csrc/common.h Elem<T>::VEC)
BOTH = ("f32", "bf16")
PAIRS = (("f32", "bf16"), ("f32", "f32"), ("bf16", "bf16"), ("bf16", "f32"))
MP_CHUNK = 8192                                 # fod_multi_permute_chunk(): destination elements per block of a row / generic job
SENTINEL = 768.0                                # exact in bf16; what a destination buffer holds before a launch


def seed_of(name):
    return zlib.crc32(name.encode())


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ fod_multi_permute3
# name:     unique; the tests select by it and seed their inputs from it
# src/dst:  "f32" | "bf16"
# dims:     (d0, d1, d2) of the destination;  sstr: source strides in elements;  src_off: the source is a view starting
#           that many elements into its (16-byte aligned) allocation
# dstr:     (t0, t1) destination strides (t2 = 1);  dst_off: the destination starts that many elements into its buffer
# valid1/2: indices from there on are written as zero;  axis: dim the f32 scale vector runs along (-1: no scale)
# path:     "t16" (transpose through LDS, df <= 16) | "t32" (df > 16) | "rows" | "generic"
# epi:      store epilogue of the column tiles of a transposing job: "vec16" | "scalar" | "both" (some tiles each)
# why:      for a generic job with a unit source stride along dim 2, the one rows-path condition that fails
# share:    jobs with the same key write slots of one destination buffer
Permute = namedtuple("Permute", "name src dst dims sstr src_off dstr dst_off valid1 valid2 axis path epi why share")
PERMUTE = []


def _perm(name, dims, sstr, path, *, src="f32", dst="bf16", src_off=0, dstr=None, dst_off=0, valid1=None, valid2=None,
          axis=-1, epi=None, why=None, share=None):
    d0, d1, d2 = dims
    assert all(p.name != name for p in PERMUTE), name
    PERMUTE.append(Permute(name, src, dst, tuple(dims), tuple(sstr), src_off, tuple(dstr) if dstr else (d1 * d2, d2),
                           dst_off, d1 if valid1 is None else valid1, d2 if valid2 is None else valid2, axis, path, epi,
                           why, share))


def oihw(cout, cin, cpad=None):
    """OIHW 3x3 weights read as [Cout][tap][Cin]: (dims, source strides)."""
    return (cout, 9, cin if cpad is None else cpad), (9 * cin, 1, 9)


def transpose2d(K, N, d0=1):
    """[d0][N][K] read as [d0][K][N]."""
    return (d0, K, N), (N * K if d0 > 1 else 0, 1, K)


def rows3(d0, d1, d2, row=None):
    """A contiguous [d0][d1][row >= d2] source read in place."""
    row = d2 if row is None else row
    return (d0, d1, d2), (d1 * row, row, 1)


def _epi_of(dst, d2):
    """With the contiguous destination (t1 = d2, t0 a multiple of it)."""
    if dst != "bf16" or d2 < 256 or d2 % 8:
        return "scalar"
    return "vec16" if d2 % 256 == 0 else "both"


# ---- transpose, df <= 16
for _co, _ci in ((5, 24), (3, 256), (2, 300)):
    for _s, _d in PAIRS if (_co, _ci) == (3, 256) else PAIRS[:2]:
        _perm(f"t16-oihw-{_co}x{_ci}-{_s}-{_d}", *oihw(_co, _ci), "t16", src=_s, dst=_d, axis=0, epi=_epi_of(_d, _ci))
_perm("t16-oihw-2x264", *oihw(2, 264), "t16", axis=0, epi="both")
_perm("t16-oihw-2x300-rows-of-304", *oihw(2, 300), "t16", dstr=(9 * 304, 304), axis=2, epi="both")
_perm("t16-fast0-d0=7", (7, 3, 20), (1, 140, 7), "t16", epi="scalar", axis=1)           # [3][20][7] read as [7][3][20]
_perm("t16-df=16", (2, 16, 40), (640, 1, 16), "t16", epi="scalar", axis=2)
_perm("t16-cin3-padded-to-8", *oihw(4, 3, 8), "t16", valid2=3, axis=0, epi="scalar")
_perm("t16-cin3-padded-to-8-f32", *oihw(4, 3, 8), "t16", dst="f32", valid2=3, axis=0, epi="scalar")
# ---- transpose, df > 16: partial last f-tile (17, 33, 40), partial last column tile (8, 255, 264, 300, 520), a full
# tile followed by a partial one in both directions
for _K, _N in itertools.product((17, 32, 33, 40), (8, 255, 256, 264, 300, 520)):
    _perm(f"t32-{_K}x{_N}", *transpose2d(_K, _N), "t32", epi=_epi_of("bf16", _N),
          axis=(-1, 1, 2)[(_K + _N) % 3])
for _s, _d in PAIRS[1:]:
    _perm(f"t32-33x264-{_s}-{_d}", *transpose2d(33, 264), "t32", src=_s, dst=_d, epi=_epi_of(_d, 264), axis=2)
_perm("t32-d0=3", *transpose2d(33, 264, d0=3), "t32", epi="both", axis=0)
_perm("t32-valid1", *transpose2d(40, 300), "t32", valid1=33, epi="scalar", axis=1)      # t1 = 300: not a multiple of 8
_perm("t32-valid2", *transpose2d(40, 520), "t32", valid2=515, epi="both", axis=2)
# ---- the 16-byte-store epilogue and each of its fallbacks, at one shape
_perm("epi-all-met", *transpose2d(40, 520), "t32", epi="both", axis=2)
_perm("epi-all-met-512", *transpose2d(40, 512), "t32", epi="vec16", axis=2)
_perm("epi-t1-not-8", *transpose2d(40, 520), "t32", dstr=(40 * 524, 524), epi="scalar", axis=2)
_perm("epi-dst-8-byte-aligned", *transpose2d(40, 520), "t32", dst_off=4, epi="scalar", axis=2)
_perm("epi-d2=300", *transpose2d(40, 300), "t32", dstr=(40 * 304, 304), epi="both", axis=2)
_perm("epi-f32-dst", *transpose2d(40, 520), "t32", dst="f32", epi="scalar", axis=2)
# ---- rows
for _d in BOTH:
    for _ax in (-1, 0, 1, 2):
        _perm(f"rows-3x50x68-{_d}-axis{_ax}", *rows3(3, 50, 68), "rows", dst=_d, axis=_ax)
    _perm(f"rows-8192-{_d}", (1, 1, 8192), (0, 0, 1), "rows", dst=_d, axis=2)
    _perm(f"rows-8196-{_d}", (1, 1, 8196), (0, 0, 1), "rows", dst=_d)
    _perm(f"rows-valid1-{_d}", *rows3(2, 12, 16), "rows", dst=_d, valid1=9, axis=1)
    _perm(f"rows-valid2-{_d}", *rows3(2, 5, 16), "rows", dst=_d, valid2=12, axis=2)
    _perm(f"rows-dstr-{_d}", *rows3(3, 50, 68), "rows", dst=_d, dstr=(50 * 72 + 8, 72), dst_off=8, axis=0)
_perm("rows-source-row-longer", *rows3(3, 5, 8, row=12), "rows", valid2=8)
# ---- generic: one case for each rows-path condition that fails, and a job without any unit stride
_perm("generic-d2=3", (4, 5, 3), (20, 4, 1), "generic", dstr=(20, 4), why="d2 % 4", axis=2)     # (valid2 = d2 fails with it)
_perm("generic-valid2=6", *rows3(2, 5, 8), "generic", valid2=6, why="valid2 % 4", axis=2)
_perm("generic-bf16-source", *rows3(3, 50, 68), "generic", src="bf16", why="f32 source", axis=1)
_perm("generic-bf16-source-f32", *rows3(3, 50, 68), "generic", src="bf16", dst="f32", why="f32 source", axis=0)
_perm("generic-source-one-element-in", *rows3(3, 50, 68), "generic", src_off=1, why="source alignment")
_perm("generic-s0-not-4", (3, 5, 8), (42, 8, 1), "generic", why="s0 % 4", axis=0)
_perm("generic-s1-not-4", (3, 5, 8), (52, 10, 1), "generic", why="s1 % 4")
_perm("generic-t1-not-4", *rows3(3, 5, 8), "generic", dstr=(52, 10), why="t1 % 4", axis=2)
_perm("generic-t0-not-4", *rows3(3, 5, 8), "generic", dstr=(42, 8), why="t0 % 4")
_perm("generic-dst-8-byte-aligned", *rows3(3, 5, 8), "generic", dst="f32", dst_off=2, why="destination alignment")
_perm("generic-no-unit-stride", (3, 4, 5), (40, 10, 2), "generic", axis=1)
_perm("generic-no-unit-stride-2-chunks", (3, 60, 50), (2, 6, 360), "generic", src="bf16", dst="f32", axis=2)
# ---- two jobs that write different slots of one buffer (stacked linears: rows of a [2 * 24][40] table; column
# blocks of a [40][2 * 24] table), as the stacked projections do
_perm("slot-rows-0", *rows3(1, 24, 40), "rows", share="stack", dstr=(0, 40), dst_off=0)
_perm("slot-rows-1", *rows3(1, 24, 40), "rows", share="stack", dstr=(0, 40), dst_off=24 * 40, axis=1)
_perm("slot-cols-0", *transpose2d(40, 24), "t32", share="stack_t", dstr=(0, 48), dst_off=0, epi="scalar")
_perm("slot-cols-1", *transpose2d(40, 24), "t32", share="stack_t", dstr=(0, 48), dst_off=24, epi="scalar", axis=2)

MIXED_TABLE = ("t16-oihw-5x24-f32-bf16", "rows-3x50x68-bf16-axis2", "t32-33x300", "generic-no-unit-stride", "slot-rows-0",
               "epi-all-met", "slot-cols-1", "t16-cin3-padded-to-8", "rows-8196-f32", "slot-rows-1", "generic-bf16-source",
               "slot-cols-0", "t32-33x264-bf16-f32", "rows-valid1-bf16")


def permute(name):
    (c,) = [p for p in PERMUTE if p.name == name]
    return c


def src_span(c):
    """Elements of the source allocation a job's full (d0, d1, d2) index range spans, from its first element."""
    return 1 + sum((d - 1) * s for d, s in zip(c.dims, c.sstr))


def dst_span(c):
    return 1 + (c.dims[0] - 1) * c.dstr[0] + (c.dims[1] - 1) * c.dstr[1] + c.dims[2] - 1


def dst_numel(c):
    """Elements of the case's destination buffer: its slot and 16 sentinels behind it (shared buffers: the largest)."""
    own = lambda p: p.dst_off + dst_span(p) + 16
    return max(own(p) for p in PERMUTE if p.share == c.share) if c.share else own(c)


def is_single_call(c):
    """Expressible as one fod_permute3_cast call: no valid1, a contiguous destination."""
    return c.valid1 == c.dims[1] and c.dstr == (c.dims[1] * c.dims[2], c.dims[2])


# ---- the rule of include/fod.h and csrc/elementwise.hip, stated in Python
def fast_dim(dims, sstr):
    """mp_fast_dim: the destination dim along which the source is contiguous."""
    if sstr[2] == 1 or dims[2] == 1:
        return 2
    if sstr[1] == 1 and dims[1] > 1:
        return 1
    if sstr[0] == 1 and dims[0] > 1:
        return 0
    return -1


def permute_tiles(dims, sstr):
    """fod_multi_permute_tiles: blocks a job takes."""
    f = fast_dim(dims, sstr)
    if f in (0, 1):
        df, dg = (dims[1], dims[0]) if f == 1 else (dims[0], dims[1])
        return cdiv(dims[2], 256) * cdiv(df, 32) * dg
    n = dims[0] * dims[1] * dims[2]
    return -1 if n >= 2 ** 31 else cdiv(n, MP_CHUNK)


def rows_conditions(c):
    """Every condition of multi_permute_body's rows path, by name (allocations are 16-byte aligned)."""
    return {"unit stride along dim 2": fast_dim(c.dims, c.sstr) == 2, "d2 % 4": c.dims[2] % 4 == 0,
            "valid2 % 4": c.valid2 % 4 == 0, "f32 source": c.src == "f32",
            "source alignment": c.src_off * ESIZE[c.src] % 16 == 0, "s0 % 4": c.sstr[0] % 4 == 0,
            "s1 % 4": c.sstr[1] % 4 == 0, "t0 % 4": c.dstr[0] % 4 == 0, "t1 % 4": c.dstr[1] % 4 == 0,
            "destination alignment": c.dst_off * ESIZE[c.dst] % 16 == 0}


def permute_path(c):
    """(path, epilogue) multi_permute_body takes for the case."""
    f = fast_dim(c.dims, c.sstr)
    if f in (0, 1):
        df = c.dims[1] if f == 1 else c.dims[0]
        vec = [c.dst == "bf16" and c0 + 256 <= c.dims[2] and (c.dstr[0] | c.dstr[1]) % 8 == 0
               and c.dst_off * ESIZE[c.dst] % 16 == 0 for c0 in range(0, c.dims[2], 256)]
        return "t16" if df <= 16 else "t32", "vec16" if all(vec) else "both" if any(vec) else "scalar"
    return ("rows" if all(rows_conditions(c).values()) else "generic"), None


# ------------------------------------------------------------------------------------------------ fod_eltwise
EW_OPS = ("ADD", "MUL", "RELU_MASK", "SCALE", "ADD3", "RELU", "COPY_B")          # the order of lib.EW_*
EW_NEEDS_B = ("ADD", "MUL", "RELU_MASK", "ADD3", "COPY_B")
EW_SHAPES = ((1, 8), (37, 64), (12, 100), (5, 7), (300, 256))
EW_OPERANDS = ("aligned", "a+1", "out+1", "b+1")          # which operand is a view starting one element into its buffer
EW_BCAST = {"none": (0, 0), "mod": (0, 4), "div": (3, 0), "div-mod": (3, 4)}     # (b_row_div, b_row_mod)
EW_ALPHAS = (2.0, -0.5)


def eltwise_kernel(dtype, shape, operand, has_b):
    """"vec" | "scalar": fod_eltwise takes the 16-byte kernel when the row length is a multiple of the vector width and
    every operand it is given is 16-byte aligned."""
    off = operand != "aligned" and (has_b or operand != "b+1")
    return "vec" if shape[1] % VEC[dtype] == 0 and not off else "scalar"


def eltwise_b_rows(rows, div, mod):
    """Rows of b the call reads (what ops.eltwise asks for)."""
    need = (rows - 1) // div + 1 if div else rows
    return min(need, mod) if mod else need


# ------------------------------------------------------------------------------------------------ fod_permute3_cast
# (dims, strides, valid2): padded OIHW-like, a transposed read, one that needs several blocks
P3_SHAPES = (((6, 5, 8), (15, 3, 1), 3), ((3, 5, 6), (1, 3, 15), None), ((7, 33, 40), (33 * 36, 1, 33), 36),
             ((2, 9, 300), (2700, 300, 1), None))
P3_AXES = (-1, 0, 1, 2)

# ------------------------------------------------------------------------------------------------ layout
# fod_nchw_to_nhwc, (F, C, H, W), Cp, dtype, the kernel: "px4" (bf16, Cp = 8, H * W % 4 == 0: four pixels per thread)
NCHW = (((3, 3, 12, 14), 8, "bf16", "px4"), ((1, 1, 2, 2), 8, "bf16", "px4"), ((2, 8, 6, 10), 8, "bf16", "px4"),
        ((3, 3, 10, 13), 8, "bf16", "general"), ((2, 3, 4, 6), 4, "bf16", "general"), ((2, 3, 4, 6), 16, "bf16", "general"),
        ((2, 3, 4, 6), 8, "f32", "general"), ((3, 3, 12, 14), 4, "f32", "general"))
# ops.clip_to_nhwc_frame_major: (B, L of the allocation, (first, last) frame of the clip handed over, C, H, W)
CLIPS = ((2, 3, None, 3, 6, 10), (3, 1, None, 3, 6, 10), (2, 5, (1, 4), 3, 6, 10), (2, 3, None, 3, 5, 7),
         (2, 5, (1, 4), 3, 5, 7), (3, 1, None, 1, 2, 2))
CLIP_OUT = (("f32", 4), ("bf16", 8), ("bf16", 4))          # (dtype, Cp)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def nchw_kernel(C, H, W, Cp, dtype, stride_outer, stride_inner, src_off):
    ok = dtype == "bf16" and Cp == 8 and H * W % 4 == 0 and stride_outer % 4 == 0 and stride_inner % 4 == 0 and src_off % 4 == 0
    return "px4" if ok else "general"


def clip_kernel(clip, dtype, cp, source):
    B, L, cut, C, H, W = clip
    if source == "u8":
        return "u8"
    return nchw_kernel(C, H, W, cp, dtype, C * H * W, L * C * H * W, cut[0] * C * H * W if cut else 0)


# ------------------------------------------------------------------------------------------------ fod_maxpool3x3s2
POOL_HW = (1, 2, 7, 8)
POOL = (("f32", 8, "vec"), ("f32", 12, "vec"), ("f32", 6, "scalar"), ("bf16", 16, "vec"), ("bf16", 6, "scalar"),
        ("bf16", 12, "scalar"))


def pool_kernel(dtype, C):
    return "vec" if C % VEC[dtype] == 0 else "scalar"


# ------------------------------------------------------------------------------------------------ fod_colsum_groups_multi
COLSUM_ROWS = (1, 3, 4, 5, 28, 29, 32, 33, 61, 100)
COLSUM_N = (4, 64, 252, 256)
# (jobs, groups, group_rows, N): every group_rows meets N = 252, every N meets group_rows = 33
COLSUM = tuple((3 if i % 2 else 1, 5 if i % 3 else 1, gr, 252) for i, gr in enumerate(COLSUM_ROWS)) + \
    ((1, 1, 33, 4), (16, 1, 33, 64), (3, 5, 33, 256), (16, 5, 100, 256), (16, 5, 29, 4), (3, 1, 61, 64))


def colsum_trips(group_rows):
    """(trips of the 32-row loop, trips of the 4-row tail) of each of the four row lanes rl = 0 .. 3."""
    out = []
    for rl in range(4):
        m, big, tail = rl, 0, 0
        while m + 28 < group_rows:
            m, big = m + 32, big + 1
        while m < group_rows:
            m, tail = m + 4, tail + 1
        out.append((big, tail))
    return out


# ------------------------------------------------------------------------------------------------ heads, optimizer
HEAD_D = (128, 256)
HEAD_REF_ROWS = (1, 7, 40, 130)
HEAD_SHARED = (1, 3)                             # rows of t per reference point (R = shared * ref_rows)
HEAD_SATURATED = ((20.0, -20.0), (-20.0, 20.0))  # logits whose f32 sigmoid is 1 / below the clamp of inverse_sigmoid

ADAMW_CHUNK = 16384
# (elements, offset of the parameter / gradient / first / second moment view into its buffer, in elements)
ADAMW_TENSORS = ((3, 0, 0, 0, 0), (16383, 1, 0, 0, 0), (16384, 0, 0, 0, 0), (16385, 2, 2, 0, 0), (16387, 0, 0, 0, 0),
                 (40000, 3, 1, 0, 0), (16385, 0, 1, 0, 0), (40000, 0, 0, 0, 0), (16385, 0, 0, 1, 0), (3, 0, 0, 0, 2))
ADAMW_SIZES = (3, 16383, 16384, 16385, 16387, 40000)


def adamw_path(t):
    n, po, go, mo, vo = t
    return "vec" if (po | go | mo | vo) % 4 == 0 else "scalar"


def sqnorm_path(t):
    return "vec" if t[2] % 4 == 0 else "scalar"
