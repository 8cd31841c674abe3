"""What tests/test_layout_gpu.py relies on, checked without a GPU: the planner of fod_multi_permute3 against the rule of
include/fod.h and csrc/elementwise.hip stated in Python, the job table the production host code builds from it, and --
for every case of tests/layout_cases.py -- that the path written in the table is the one a Python statement of the
kernel's conditions gives, with a census per path so that no path is left without a case."""
import collections
import ctypes
import random

import pytest
import torch

import layout_cases as LC
from future_od.native import functional as Fn
from future_od.native import lib as L


def _tiles(dims, sstr):
    return int(L.LIB.fod_multi_permute_tiles(dims[0], dims[1], dims[2], sstr[0], sstr[1], sstr[2]))


def test_chunk_constants():
    assert int(L.LIB.fod_multi_permute_chunk()) == LC.MP_CHUNK and int(L.LIB.fod_multi_chunk()) == LC.ADAMW_CHUNK
    assert [getattr(L, "EW_" + n) for n in LC.EW_OPS] == list(range(7))


def test_permute_planner_follows_the_stated_rule():
    """fod_multi_permute_tiles: the fast dim as mp_fast_dim chooses it; ceil(d2 / 256) * ceil(df / 32) * dg blocks for a
    transposing job, ceil(n / 8192) otherwise, -1 from 2^31 elements on."""
    for c in LC.PERMUTE:
        assert _tiles(c.dims, c.sstr) == LC.permute_tiles(c.dims, c.sstr) > 0, c.name
    rng = random.Random(7)
    kinds = collections.Counter()
    for _ in range(400):
        dims = tuple(rng.choice((1, 1, 2, 3, 9, 16, 17, 32, 33, 64, 255, 256, 257, 300, 1000)) for _ in range(3))
        sstr = tuple(rng.choice((0, 1, 1, 2, 9, 33, 256, 4096)) for _ in range(3))
        want = LC.permute_tiles(dims, sstr)
        assert _tiles(dims, sstr) == want, (dims, sstr)
        kinds[LC.fast_dim(dims, sstr)] += 1
    assert all(kinds[f] >= 20 for f in (-1, 0, 1, 2)), kinds
    contiguous = lambda d: (d[1] * d[2], d[2], 1)
    for dims, want in (((2048, 1024, 1024), -1), ((2047, 1024, 1024), 2047 * 128), ((1, 1, 8192), 1), ((1, 1, 8193), 2)):
        assert _tiles(dims, contiguous(dims)) == LC.permute_tiles(dims, contiguous(dims)) == want
    # a transposing job is counted in tiles whatever its element count
    assert _tiles((1, 65536, 32768), (0, 1, 65536)) == LC.permute_tiles((1, 65536, 32768), (0, 1, 65536)) == 128 * 2048


def _cpu_job(c, scale=None):
    src = torch.zeros(c.src_off + LC.src_span(c), dtype=LC.DTYPE[c.src])
    dst = torch.zeros(LC.dst_numel(c), dtype=LC.DTYPE[c.dst])
    if scale is None and c.axis >= 0:
        scale = torch.ones(c.dims[c.axis])
    return Fn._Job(src[c.src_off:], dst[c.dst_off:], c.dims, c.sstr, dstr=c.dstr, valid1=c.valid1, valid2=c.valid2,
                   scale=scale, axis=c.axis)


def test_build_tables_emits_one_block_per_tile_in_order():
    """Fn._Prepared._build_tables: exactly fod_multi_permute_tiles (job, chunk) pairs per job, jobs in order, chunks
    0 .. n-1, and a job record that says what the _Job said."""
    jobs = [_cpu_job(c) for c in LC.PERMUTE]
    raw, blk_job, blk_chunk, nblocks, keep = Fn._Prepared()._build_tables(jobs)
    want_job, want_chunk = [], []
    for i, c in enumerate(LC.PERMUTE):
        n = LC.permute_tiles(c.dims, c.sstr)
        want_job += [i] * n
        want_chunk += range(n)
    assert nblocks == len(want_job) and blk_job.dtype == torch.int32 and blk_chunk.dtype == torch.int32
    assert blk_job.tolist() == want_job and blk_chunk.tolist() == want_chunk
    assert len(keep) == len(jobs) and raw.numel() == len(jobs) * ctypes.sizeof(L.PermuteJob)
    recs = (L.PermuteJob * len(jobs)).from_buffer_copy(raw.numpy().tobytes())
    names = [f[0] for f in L.PermuteJob._fields_]
    for c, j, r in zip(LC.PERMUTE, jobs, recs):
        got = tuple(getattr(r, n) or 0 for n in names)
        want = (j.src.data_ptr(), j.dst.data_ptr(), 0 if j.scale is None else j.scale.data_ptr(), L.F32 if c.src == "f32" else L.BF16,
                L.F32 if c.dst == "f32" else L.BF16) + c.dims + (c.valid1, c.valid2, c.axis) + c.sstr + c.dstr
        assert got == want, (c.name, names, got, want)


def test_build_tables_wants_an_aligned_scale_on_the_rows_path():
    """The rows path reads a scale along dim 2 with a 16-byte load: the host refuses a misaligned one for exactly the jobs
    that take that path (its statement of the kernel's condition agrees with the table's for every case); transposing
    and generic jobs read the scale element by element and may have it."""
    for c in LC.PERMUTE:
        assert Fn._Prepared._takes_rows_path(_cpu_job(c)) == (c.path == "rows"), c.name
    off = lambda c: torch.ones(c.dims[2] + 1)[1:]
    for c in LC.PERMUTE:
        if c.axis != 2:
            continue
        assert off(c).data_ptr() % 16 == 4
        if c.path == "rows":
            with pytest.raises(L.FodError, match="16-byte aligned"):
                Fn._Prepared()._build_tables([_cpu_job(c, off(c))])
        else:
            Fn._Prepared()._build_tables([_cpu_job(c, off(c))])
    assert {c.path for c in LC.PERMUTE if c.axis == 2} == {"t16", "t32", "rows", "generic"}


# ------------------------------------------------------------------------------------------------ every path has a case
def test_permute_cases_take_the_paths_the_table_says():
    census = collections.Counter()
    for c in LC.PERMUTE:
        assert LC.permute_path(c) == (c.path, c.epi), (c.name, LC.permute_path(c))
        assert c.axis == -1 or 0 <= c.axis <= 2
        census[c.path] += 1
        census[c.path, c.src, c.dst] += 1
        if c.epi:
            census[c.path, c.epi] += 1
        if c.path == "generic" and LC.fast_dim(c.dims, c.sstr) == 2:
            failing = {k for k, ok in LC.rows_conditions(c).items() if not ok}
            assert failing == {c.why} or (c.why == "d2 % 4" and failing == {"d2 % 4", "valid2 % 4"}), (c.name, failing)
            census["generic because", c.why] += 1
        if c.path in ("rows", "generic"):
            census[c.path, "chunks", min(LC.permute_tiles(c.dims, c.sstr), 2)] += 1
            census[c.path, "axis", c.axis] += 1
        else:
            census["transpose", "fast dim", LC.fast_dim(c.dims, c.sstr)] += 1
            census[c.path, "axis", c.axis] += 1
        for what, on in (("valid1", c.valid1 < c.dims[1]), ("valid2", c.valid2 < c.dims[2]),
                         ("dstr", c.dstr != (c.dims[1] * c.dims[2], c.dims[2])), ("dst_off", c.dst_off > 0)):
            if on:
                census[c.path, what] += 1
        census["single call", LC.is_single_call(c)] += 1
    need = [p for p in ("t16", "t32", "rows", "generic")]
    need += [(p, e) for p in ("t16", "t32") for e in ("vec16", "scalar", "both")]
    need += [(p, s, d) for p in ("t16", "t32", "generic") for s, d in LC.PAIRS] + [("rows", "f32", d) for d in LC.BOTH]
    need += [("generic because", k) for k in LC.rows_conditions(LC.PERMUTE[0]) if k != "unit stride along dim 2"]
    need += [(p, "axis", a) for p in ("t16", "t32", "rows", "generic") for a in (0, 1, 2)] + [("rows", "axis", -1), ("t32", "axis", -1)]
    need += [(p, "chunks", n) for p in ("rows", "generic") for n in (1, 2)]
    need += [("transpose", "fast dim", 0), ("transpose", "fast dim", 1)]
    need += [("t16", "valid2"), ("t32", "valid1"), ("t32", "valid2"), ("rows", "valid1"), ("rows", "valid2"), ("rows", "dstr"),
             ("rows", "dst_off"), ("t32", "dstr"), ("t32", "dst_off"), ("generic", "dstr"), ("single call", True)]
    missing = [k for k in need if census[k] == 0]
    assert not missing, missing
    mixed = [LC.permute(n) for n in LC.MIXED_TABLE]
    assert collections.Counter(c.share for c in mixed if c.share) == {"stack": 2, "stack_t": 2}
    # slots of a shared buffer do not overlap
    for key in ("stack", "stack_t"):
        cells = collections.Counter()
        for c in (c for c in LC.PERMUTE if c.share == key):
            cells.update(torch.as_strided(torch.arange(LC.dst_numel(c)), c.dims, c.dstr + (1,), c.dst_off).flatten().tolist())
        assert max(cells.values()) == 1, key


def test_every_other_kernel_of_the_table_is_reached():
    census = collections.Counter()
    for dtype in LC.BOTH:
        for shape in LC.EW_SHAPES:
            for operand in LC.EW_OPERANDS:
                census["eltwise", dtype, LC.eltwise_kernel(dtype, shape, operand, True)] += 1
                census["eltwise", shape, dtype, LC.eltwise_kernel(dtype, shape, operand, True)] += 1
    assert LC.eltwise_kernel("f32", (12, 100), "aligned", True) == "vec" and LC.eltwise_kernel("bf16", (12, 100), "aligned", True) == "scalar"
    assert all(LC.eltwise_kernel(d, (5, 7), "aligned", True) == "scalar" for d in LC.BOTH)
    assert LC.eltwise_kernel("f32", (37, 64), "b+1", False) == "vec"             # an op without b is not given the view
    for shape in LC.EW_SHAPES:
        for div, mod in LC.EW_BCAST.values():
            used = {(m // div if div else m) % mod if mod else (m // div if div else m) for m in range(shape[0])}
            assert used == set(range(LC.eltwise_b_rows(shape[0], div, mod))), (shape, div, mod)
    for (f, c, h, w), cp, dtype, kernel in LC.NCHW:
        assert LC.nchw_kernel(c, h, w, cp, dtype, c * h * w, 0, 0) == kernel and cp >= c
        census["nchw", kernel] += 1
        if kernel == "general":
            census["nchw general because", "hw" if h * w % 4 else "cp" + str(cp) if cp != 8 else dtype] += 1
    for clip in LC.CLIPS:
        for dtype, cp in LC.CLIP_OUT:
            for source in ("f32", "u8"):
                if cp >= clip[3]:
                    census["clip", LC.clip_kernel(clip, dtype, cp, source), "cut" if clip[2] else "whole", dtype] += 1
    for dtype, C, kernel in LC.POOL:
        assert LC.pool_kernel(dtype, C) == kernel
        census["pool", dtype, kernel] += 1
    for jobs, groups, gr, N in LC.COLSUM:
        assert jobs in (1, 3, 16) and groups in (1, 5) and gr in LC.COLSUM_ROWS and N in LC.COLSUM_N and N % 4 == 0
        census["colsum jobs", jobs] += 1
        census["colsum groups", groups] += 1
        for big, tail in LC.colsum_trips(gr):
            census["colsum trips", min(big, 2), min(tail, 2)] += 1
            census["colsum 32-row trips", min(big, 2)] += 1
            census["colsum 4-row trips", min(tail, 2)] += 1
    assert {gr for _, _, gr, N in LC.COLSUM if N == 252} == set(LC.COLSUM_ROWS)
    assert {N for _, _, gr, N in LC.COLSUM if gr == 33} == set(LC.COLSUM_N)
    for t in LC.ADAMW_TENSORS:
        census["adamw", LC.adamw_path(t), "tail" if t[0] % 4 else "whole"] += 1
        census["sqnorm", LC.sqnorm_path(t)] += 1
        census["adamw chunks", min(LC.cdiv(t[0], LC.ADAMW_CHUNK), 3)] += 1
    need = [("eltwise", d, k) for d in LC.BOTH for k in ("vec", "scalar")]
    need += [("nchw", "px4"), ("nchw", "general")] + [("nchw general because", k) for k in ("hw", "cp4", "cp16", "f32")]
    need += [("clip", k, cut, d) for k, d in (("px4", "bf16"), ("general", "f32"), ("general", "bf16"), ("u8", "f32"), ("u8", "bf16"))
             for cut in ("cut", "whole")]
    need += [("pool", d, k) for d in LC.BOTH for k in ("vec", "scalar")]
    need += [("colsum jobs", j) for j in (1, 3, 16)] + [("colsum groups", g) for g in (1, 5)]
    need += [("colsum 32-row trips", n) for n in (0, 1, 2)] + [("colsum 4-row trips", n) for n in (0, 1, 2)]
    need += [("colsum trips", 0, 1), ("colsum trips", 0, 2), ("colsum trips", 1, 0), ("colsum trips", 1, 1), ("colsum trips", 2, 0)]
    need += [("adamw", "vec", "tail"), ("adamw", "vec", "whole"), ("adamw", "scalar", "tail"), ("sqnorm", "vec"),
             ("sqnorm", "scalar"), ("adamw chunks", 1), ("adamw chunks", 2), ("adamw chunks", 3)]
    missing = [k for k in need if census[k] == 0]
    assert not missing, missing


def test_oracle_gradients_are_finite_at_the_saturated_logits():
    """The inputs test_layout_gpu.py adds to the box-head case: the oracle's own autograd through sigmoid, the sine
    embedding and inverse_sigmoid(eps=1e-5) stays finite there (the clamps of inverse_sigmoid cut the gradient, they do
    not divide by zero), in float64 and from float32 / bfloat16-rounded logits alike."""
    from oracle import stdetr as O
    from oracle import thirdparty as tp
    for dtype in (torch.float64, torch.float32):
        logit = torch.tensor(LC.HEAD_SATURATED, dtype=dtype).requires_grad_(True)
        assert torch.equal(logit.detach().to(torch.bfloat16).to(dtype), logit.detach())
        ref = logit.sigmoid()
        out = O.query_sine_embed(ref[:, None, :], 128)[:, 0].sum() + (tp.inverse_sigmoid(ref) + 0.5).sigmoid().sum()
        (grad,) = torch.autograd.grad(out, logit)
        assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(tp.inverse_sigmoid(ref)).all())
    # the f32 sigmoid the kernel computes: exactly 1 at +20, below the clamp at -20
    s = torch.tensor([20.0, -20.0]).sigmoid()
    assert float(s[0]) == 1.0 and 0.0 < float(s[1]) < 1e-5
