"""Cases, references and limits for the attention maps (include/fod_ext.h: fod_attn_maps, fod_render_attention), shared by
tests/test_attention_maps_cpu.py and tests/test_attention_maps_gpu.py.  Nothing here imports a helper of the package:
the float64 reference of the maps is plain torch on the same rounded inputs, the overlay is restated in numpy float32.

A map case is a MapCase; `build(case)` gives its operands on the CPU (bf16 cases: rounded to bf16 first, so that the
kernel and the reference start from the same numbers), `reference(...)` the float64 maps and A, the case's largest
|score * scale * log2 e|.

The limit of a case, relative to the row maximum of the reference:   3 * d32 + 8 * 2^-24 * (1 + A)
  d32: the same statistic of a float32 torch restatement against float64, measured on the CPU and recorded in D32 below
       (tests/test_attention_maps_cpu.py measures it again); three times is the project's margin (criterion_cases.py).
  8 * 2^-24 * (1 + A): derived, not measured -- eight f32 roundings of an exponent argument of magnitude up to 1 + A (the
       folded constant scale * log2 e, the subtraction of the row maximum and of the log of the sum, that sum's own
       roundings, the 1-ulp v_exp_f32 and the head mean)."""
import math
from collections import namedtuple

import numpy as np
import torch

import render_cases as RC

LOG2E = 1.4426950408889634
MEASURED_FACTOR = 3.0
ROUNDINGS = 8 * 2.0 ** -24

MapCase = namedtuple("MapCase", "name B H Tq S Q table parts k2_per_batch strided njobs dtype gain")


def _c(name, B=2, H=8, Tq=33, S=130, Q=None, table=True, parts=2, k2_per_batch=False, strided=True, njobs=2,
       dtype="bf16", gain=1.0):
    """Q None: all of Tq.  table False: query_idx is NULL (then Q == Tq)."""
    Q = Tq if Q is None else Q
    assert table or Q == Tq
    return MapCase(name, B, H, Tq, S, Q, table, parts, k2_per_batch, strided, njobs, dtype, gain)


# The smallest shapes at which the kernel can go wrong: the key tile is 32 (S around one and two tiles, a single key, four
# tiles and a remainder), the query tile is 32 (Q 1, 31, 32, 33), and from S = 512 on the keys of the second pass are cut
# into chunks of at least 256 across workgroups when few query tiles are launched (S = 520: two chunks of 288; S = 1030
# with one query tile: four chunks of 288).
MAP_CASES = [
    _c("base"),
    _c("S1", S=1), _c("S63", S=63), _c("S64", S=64), _c("S65", S=65), _c("S33 one part f32", S=33, parts=1, dtype="f32"),
    _c("S520 two chunks", S=520, njobs=1, B=1), _c("S1030 four chunks", S=1030, njobs=1, B=1, H=1, Tq=8),
    _c("Q1 table", Q=1), _c("Q31 table", Q=31), _c("Q32 table", Q=32), _c("Q70 table: duplicates", Q=70),
    _c("Tq1 identity", Tq=1, table=False), _c("Tq31 identity", Tq=31, table=False), _c("Tq32 identity", Tq=32, table=False),
    _c("Tq33 identity", table=False),
    _c("one part", parts=1), _c("k2 per batch", k2_per_batch=True), _c("dense", strided=False),
    _c("dense k2 per batch one job", strided=False, k2_per_batch=True, njobs=1),
    _c("5 jobs", njobs=5, S=65), _c("32 jobs", njobs=32, S=33, Tq=5, H=1, B=1),
    _c("H1", H=1), _c("B1", B=1),
    _c("f32", dtype="f32"), _c("f32 dense identity", dtype="f32", strided=False, table=False),
    _c("gain4", gain=4.0), _c("gain12", gain=12.0), _c("f32 gain4", dtype="f32", gain=4.0),
    _c("f32 gain12", dtype="f32", gain=12.0), _c("f32 gain12 one part", dtype="f32", gain=12.0, parts=1),
]
BY_NAME = {c.name: c for c in MAP_CASES}
assert len(BY_NAME) == len(MAP_CASES)

# d32 of every case as measured on the CPU (measure_d32); tests/test_attention_maps_cpu.py holds them to the measurement
D32 = {
    "base": 3.12e-07, "S1": 0.0, "S63": 2.30e-07, "S64": 2.37e-07, "S65": 2.64e-07, "S33 one part f32": 4.26e-07,
    "S520 two chunks": 2.94e-07, "S1030 four chunks": 1.75e-07,
    "Q1 table": 1.63e-07, "Q31 table": 3.25e-07, "Q32 table": 2.73e-07, "Q70 table: duplicates": 3.37e-07,
    "Tq1 identity": 1.36e-07, "Tq31 identity": 2.73e-07, "Tq32 identity": 3.01e-07, "Tq33 identity": 2.23e-07,
    "one part": 2.67e-07, "k2 per batch": 2.21e-07, "dense": 2.62e-07, "dense k2 per batch one job": 2.68e-07,
    "5 jobs": 2.87e-07, "32 jobs": 2.12e-07, "H1": 3.43e-07, "B1": 2.64e-07,
    "f32": 3.70e-07, "f32 dense identity": 4.26e-07,
    # A (the largest |score * scale * log2 e|) is about 7 at gain 1, 110 at gain 4 and 1000 at gain 12, where the scores
    # of one part reach 5500: the limits there are 6e-5 and 5e-4, almost all of it the derived term
    "gain4": 1.47e-06, "gain12": 8.57e-06, "f32 gain4": 2.82e-06, "f32 gain12": 1.72e-05, "f32 gain12 one part": 1.79e-05,
}


def query_table(B, Q, Tq, seed):
    """i32 [B, Q]: a permutation of the queries per sample, repeated where Q > Tq; from four entries on the row also holds
    the padding value -1, the first index past the end (Tq) and a duplicate."""
    g = np.random.default_rng(seed)
    rows = []
    for _ in range(B):
        row = np.resize(g.permutation(Tq), Q).astype(np.int32)
        if Q >= 4:
            row[0], row[1], row[3] = -1, Tq, row[2]
        rows.append(row)
    return torch.from_numpy(np.stack(rows))


def _slot(g, B, T, E, gain, dtype, strided, index):
    """A [B, T, E] operand: dense, or column slot `index` of a [B, T, 4 * E] buffer (what MemorySide.slots() gives)."""
    if not strided:
        return (torch.randn(B, T, E, generator=g) * gain).to(dtype)
    wide = (torch.randn(B, T, 4 * E, generator=g) * gain).to(dtype)
    return wide[..., index * E:(index + 1) * E]


def build(case, seed=0):
    """-> (jobs, scale, query_idx): jobs = [(q1, q2, k1, k2)] CPU tensors of the case's dtype (q2 / k2 None with one part;
    k2 a [S, E] table shared by the batch unless k2_per_batch), query_idx i32 [B, Q] or None."""
    g = torch.Generator().manual_seed(1000 + seed + sum(map(ord, case.name)))
    dtype = torch.bfloat16 if case.dtype == "bf16" else torch.float32
    E = 32 * case.H
    jobs = []
    for j in range(case.njobs):
        q1 = _slot(g, case.B, case.Tq, E, case.gain, dtype, case.strided, 1)
        k1 = _slot(g, case.B, case.S, E, case.gain, dtype, case.strided, 2)
        q2 = k2 = None
        if case.parts == 2:
            q2 = torch.empty_strided(q1.shape, q1.stride(), dtype=dtype).copy_(torch.randn(q1.shape, generator=g) * case.gain)
            k2 = _slot(g, case.B, case.S, E, case.gain, dtype, case.strided, 3)
            if not case.k2_per_batch:
                k2 = k2[0]
        jobs.append((q1, q2, k1, k2))
    idx = query_table(case.B, case.Q, case.Tq, len(case.name)) if case.table else None
    return jobs, 1.0 / math.sqrt(32 * case.parts), idx


def reference(jobs, scale, H, query_idx=None, dtype=torch.float64):
    """(maps [B, Q, J, S] in `dtype`, A) -- the head mean of softmax((q1.k1 + q2.k2) * scale) per job, rows gathered by
    query_idx (an index outside [0, Tq) gives zeros); A = the largest |score * scale * log2 e| (float64 only, else None)."""
    out, A = [], 0.0
    for q1, q2, k1, k2 in jobs:
        B, Tq, E = q1.shape
        S = k1.shape[1]
        heads = lambda t, T: t.to(dtype).expand(B, T, E).reshape(B, T, H, 32).transpose(1, 2)
        score = heads(q1, Tq) @ heads(k1, S).transpose(-1, -2)
        if q2 is not None:
            score = score + heads(q2, Tq) @ heads(k2, S).transpose(-1, -2)
        score = score * scale
        if dtype == torch.float64:
            A = max(A, float(score.abs().max()) * LOG2E)
        p = torch.softmax(score, dim=-1).mean(1)                                   # [B, Tq, S]
        if query_idx is not None:
            ok = (query_idx >= 0) & (query_idx < Tq)
            rows = torch.gather(p, 1, query_idx.clamp(0, Tq - 1).long()[..., None].expand(-1, -1, S))
            p = rows * ok[..., None].to(dtype)
        out.append(p)
    return torch.stack(out, dim=2), (A if dtype == torch.float64 else None)


def valid_rows(query_idx, B, Q, Tq):
    """bool [B, Q]: the rows that hold a map (the others are exactly zero)."""
    if query_idx is None:
        return torch.ones(B, Q, dtype=torch.bool)
    return (query_idx >= 0) & (query_idx < Tq)


def distance(got, ref, valid):
    """The statistic every limit is stated in: the largest |got - ref| over the valid rows, relative to the maximum of
    the reference's row."""
    err = (got.double() - ref).abs() / ref.amax(dim=-1, keepdim=True).clamp_min(1e-300)
    return float(err[valid].max()) if bool(valid.any()) else 0.0


def measure_d32(case):
    jobs, scale, idx = build(case)
    ref, _ = reference(jobs, scale, case.H, idx)
    f32, _ = reference([tuple(None if t is None else t.float() for t in job) for job in jobs], scale, case.H, idx,
                       torch.float32)
    return distance(f32, ref, valid_rows(idx, case.B, case.Q, case.Tq))


def limit(d32, A):
    return MEASURED_FACTOR * d32 + ROUNDINGS * (1.0 + A)


# ---- the overlay: numpy float32, one operation per step ----------------------------------------------------------------
LUT = np.array([[2 * i, 2 * i, 255] if i <= 127 else [255, 2 * (255 - i), 2 * (255 - i)] for i in range(256)],
               dtype=np.uint8)
F = np.float32


def taps(n_out, n_in):
    f = np.arange(n_out, dtype=F) + F(0.5)
    f = f * (F(n_in) / F(n_out))
    f = f - F(0.5)
    f = np.maximum(f, F(0))
    assert f.dtype == F
    i0 = np.minimum(np.trunc(f).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    w1 = f - i0.astype(F)
    return i0, i1, F(1) - w1, w1


def colour_scale(amap):
    with np.errstate(all="ignore"):
        return F(1) / np.maximum(amap.max(), F(1e-30))


def overlay(bg, amap, cs, gain, max_alpha, lut=LUT):
    """bg uint8 [H, W, 3], amap f32 [h, w], cs f32 -> uint8 [H, W, 3]."""
    H, W, _ = bg.shape
    y0, y1, wy0, wy1 = taps(H, amap.shape[0])
    x0, x1, wx0, wx1 = taps(W, amap.shape[1])
    with np.errstate(all="ignore"):
        top = amap[y0][:, x0] * wx0 + amap[y0][:, x1] * wx1
        bot = amap[y1][:, x0] * wx0 + amap[y1][:, x1] * wx1
        a = top * wy0[:, None] + bot * wy1[:, None]
        assert a.dtype == F
        alpha = a * F(gain)
        alpha = np.minimum(np.where(alpha >= 0, alpha, F(0)), F(max_alpha))
        level = a * F(cs)
        level = np.minimum(np.where(level >= 0, level, F(0)), F(1)) * F(255)
        colour = lut[np.trunc(level).astype(np.int64)].astype(F)                   # [H, W, 3]
        keep = F(1) - alpha
        mixed = bg.astype(F) * keep[..., None] + colour * alpha[..., None]
        assert mixed.dtype == F
        mixed = np.trunc(np.minimum(np.maximum(mixed, F(0)), F(255)))
        mixed = np.where(np.isfinite(a)[..., None], mixed, bg.astype(F))
    return mixed.astype(np.uint8)


def overlay_expected(case):
    """uint8 [B, J, H, W, 3] of an overlay case."""
    video, att, frames, slot = case["video"], case["attention"], case["frames"], case["slot"]
    B, L = video.shape[:2]
    out = []
    for b in range(B):
        k = slot if isinstance(slot, int) else int(slot[b])
        for j, f in enumerate(frames):
            f = min(max(f + L if f < 0 else f, 0), L - 1)
            amap = att[b, k, j]
            out.append(overlay(RC.background(video[b, f]), amap, colour_scale(amap), case["gain"], case["max_alpha"]))
    return np.stack(out).reshape(B, len(frames), *out[0].shape)


def _overlay_case(name, H, W, h, w, B=2, L=3, K=3, frames=(0,), slot=1, u8=False, gain=50.0, max_alpha=0.4, seed=0,
                  poison=False):
    g = np.random.default_rng(seed)
    video = g.integers(0, 256, (B, L, 3, H, W), dtype=np.uint8) if u8 else \
        g.standard_normal((B, L, 3, H, W)).astype(np.float32)
    # maps like a softmax row: non-negative, a few strong cells, 1 / (h * w) on average
    att = (g.random((B, K, len(frames), h, w)) ** 4).astype(np.float32)
    att = (att / att.sum(axis=(3, 4), keepdims=True)).astype(np.float32)
    if poison:
        att[0, :, 0, 0, 0] = np.nan
        att[-1, :, -1, -1, -1] = np.inf
        att[0, :, -1, 0, -1] = -0.25
    return dict(name=f"{name} {H}x{W} map {h}x{w} J{len(frames)}{' u8' if u8 else ''}", video=video, attention=att,
                frames=list(frames), slot=slot, gain=gain, max_alpha=max_alpha)


def overlay_cases():
    out = []
    for u8 in (False, True):
        out += [
            _overlay_case("one cell", 7, 9, 1, 1, u8=u8, seed=1),
            _overlay_case("small", 7, 9, 2, 3, u8=u8, frames=(0, -1, 1), seed=2),
            _overlay_case("aligned", 64, 96, 2, 3, u8=u8, frames=(2, -3, -1), slot=np.array([2, 0], dtype=np.int32), seed=3),
            _overlay_case("frames out of range", 7, 9, 2, 3, u8=u8, frames=(-9, 7, -2), B=1, seed=4),
            _overlay_case("NaN, inf and a negative cell", 7, 9, 2, 3, u8=u8, frames=(1, 0, 2), poison=True, seed=5),
            _overlay_case("gain 0", 64, 96, 2, 3, u8=u8, gain=0.0, seed=6),
            _overlay_case("max_alpha 0", 7, 9, 2, 3, u8=u8, max_alpha=0.0, frames=(0, 1, 2), seed=7),
            _overlay_case("two tile columns", 18, 262, 5, 11, u8=u8, B=1, frames=(1,), slot=0, seed=8),
        ]
    return out
