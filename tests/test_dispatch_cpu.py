"""Kernel selection, the parts that need no GPU: the knob table (csrc/knobs.h: set / get / reset, read from the
environment once), the routes the library reports for the shapes DESIGN.md §3 describes in words, and the two places
where future_od/native/ops.py must predict a route in order to hand over scratch, held against the library's answer."""
import os
import subprocess
import sys

import pytest
import torch

from future_od.native import lib as L
from future_od.native import ops

import variant_cases as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "future-object-detection_amd")
C_KNOBS = ["FOD_NT_SMALL", "FOD_NT_NARROW", "FOD_NT_SPLITK", "FOD_NT_BIG", "FOD_NT_BIG256", "FOD_NT_BIG_ILV",
           "FOD_NT_BIG256_MINK", "FOD_NT_BIG_MINK", "FOD_NT_BIG_MINN", "FOD_TN_SMALL", "FOD_TN_BIG", "FOD_TN_BIG_DENSE",
           "FOD_TN_BIG256", "FOD_TN_BIG_MIN", "FOD_TN_BIG_SPLITS", "FOD_TN_WS", "FOD_TN_XCD", "FOD_TN_ROWS", "FOD_ATTN_LDS",
           "FOD_ATTN_PF", "FOD_FP8_STAGE", "FOD_LN_BWD_GROUPS", "FOD_BNK_VERSION"]


@pytest.fixture(autouse=True)
def _default_knobs():
    """The routes below are those of the defaults, whatever the environment of this run says; put back afterwards."""
    with L.knobs(**{name: None for name in C_KNOBS}):
        yield


def test_knob_round_trip():
    assert len(C_KNOBS) == 23
    src = open(os.path.join(PKG, "csrc", "knobs.h")).read()
    for name in C_KNOBS:                              # every name is in the table, and documented in the header
        assert L.knob(name) != "" and name in src, name
    assert (L.knob("FOD_TN_BIG"), L.knob("FOD_NT_NARROW"), L.knob("FOD_TN_BIG_SPLITS")) == ("1", "auto", "0")
    assert float(L.knob("FOD_TN_BIG_MIN")) == 2.0e9
    L.set_knob("FOD_TN_BIG", 2)
    L.set_knob("FOD_TN_BIG_MIN", "1e6")
    L.set_knob("FOD_NT_NARROW", 100)
    assert (L.knob("FOD_TN_BIG"), float(L.knob("FOD_TN_BIG_MIN")), L.knob("FOD_NT_NARROW")) == ("2", 1e6, "100")
    L.set_knob("FOD_NT_NARROW", "auto")
    L.set_knob("FOD_TN_BIG", None)
    assert (L.knob("FOD_TN_BIG"), L.knob("FOD_NT_NARROW")) == ("1", "auto")
    with L.knobs(FOD_TN_BIG=0, FOD_TN_XCD=0):
        assert (L.knob("FOD_TN_BIG"), L.knob("FOD_TN_XCD")) == ("0", "0")
        with pytest.raises(L.FodError, match="unknown name"):
            L.set_knob("FOD_NO_SUCH_KNOB", 1)
        with pytest.raises(L.FodError, match="unknown name"):
            L.knob("FOD_WGRAD_QUEUE")                 # a Python-side switch: not the library's
        for bad in ("two", "", "1x", "-1", "auto"):
            with pytest.raises(L.FodError, match="cannot be"):
                L.set_knob("FOD_TN_BIG", bad)
        assert L.knob("FOD_TN_BIG") == "0"            # a refused value changes nothing
    assert (L.knob("FOD_TN_BIG"), L.knob("FOD_TN_XCD")) == ("1", "1")


def test_environment_is_read_once_at_first_use():
    """A fresh process: what the environment said when the library was first used is the initial value; what
    os.environ says afterwards is not seen (fod_knob_set is the way)."""
    code = ("import os, sys; sys.path.insert(0, sys.argv[1])\n"
            "from future_od.native import lib as L\n"
            "first = (L.knob('FOD_TN_BIG'), L.knob('FOD_NT_NARROW'), L.knob('FOD_TN_SMALL'))\n"
            "os.environ['FOD_TN_BIG'] = '0'; os.environ['FOD_TN_SMALL'] = '0'; os.environ.pop('FOD_NT_NARROW')\n"
            "print(*first, L.knob('FOD_TN_BIG'), L.knob('FOD_NT_NARROW'), L.knob('FOD_TN_SMALL'))\n")
    env = dict(os.environ, FOD_TN_BIG="2", FOD_NT_NARROW="100")
    env.pop("FOD_TN_SMALL", None)
    out = subprocess.run([sys.executable, "-c", code, PKG], env=env, check=True, capture_output=True, text=True).stdout
    assert out.split() == ["2", "100", "1", "2", "100", "1"], out


def _nt(r):
    return (r.kernel, r.tile_n, r.ksplit)


def _conv(cin, cout, k, h, w):
    return ops.conv_geom((10, h, w, cin), cout, k, 1, k // 2)


def test_default_routes_of_the_headline_shapes():
    """DESIGN.md §3 in a table.  Shapes: 10 frames at 900 x 1600 (profiles/r03q_launch_census_before.txt,
    profiles/r03q_conv_layer_rooflines.txt): layer3 at 57 x 100, layer4 at 29 x 50 = 14 500 rows, 1450 tokens per frame."""
    layer3_3x3, layer4_3x3 = _conv(256, 256, 3, 57, 100), _conv(512, 512, 3, 29, 50)
    for which in (L.CONV_FWD, L.CONV_DGRAD):
        r = ops.conv2d_route(which, layer3_3x3)
        assert (r.kernel, r.tile_n, r.stages, r.interleave) == (L.NT_BIG, 256, 2, 0)       # the 256 x 256 tile
        r = ops.conv2d_route(which, layer4_3x3)
        assert layer4_3x3.Nimg * layer4_3x3.Ho * layer4_3x3.Wo == 14500
        assert (r.kernel, r.tile_n, r.stages, r.interleave) == (L.NT_BIG, 128, 3, 1)       # 256 x 128
    # the encoder's feed-forward: the 128-row kernel
    assert _nt(ops.gemm_nt_route(14500, 2048, 256)) == (L.NT_128, 128, 1)
    assert ops.gemm_nt_route(14500, 256, 2048).kernel == L.NT_128
    # the decoder: short launches, K split four ways where it is deep
    r = ops.gemm_nt_route(256, 256, 256)
    assert _nt(r) == (L.NT_SMALL, 64, 1) and not r.wants_split_ws
    r = ops.gemm_nt_route(256, 256, 2048)
    assert _nt(r) == (L.NT_SMALL, 64, 4) and r.wants_split_ws
    assert ops.gemm_nt_route(256, 256, 2048, torch.float32).kernel == L.NT_128             # the short launch is bf16's
    # conv weight gradients with M >= 8192 and >= 2e9 MACs: the 8-wave kernel with partial tiles
    for geom in (layer3_3x3, layer4_3x3, _conv(1024, 256, 1, 57, 100), _conv(512, 2048, 1, 29, 50),
                 _conv(128, 128, 3, 113, 200)):
        M = geom.Nimg * geom.Ho * geom.Wo
        assert M >= 8192 and M * geom.Cout * geom.kh * geom.kw * geom.Cin >= 2e9
        r = ops.conv2d_route(L.CONV_WGRAD, geom)
        assert r.kernel == L.TN_BIG and r.uses_partials_ws and r.nsplit > 1 and r.xcd_order
        assert (r.bi, r.bj) in ((128, 256), (256, 128)) and r.m_per_split % 64 == 0
        assert (r.nsplit - 1) * r.m_per_split < M <= r.nsplit * r.m_per_split
    # Linear weight gradients: the 128 x 128 kernel (atomics: no partial tiles), short reductions the 64 x 64 one
    for n1, k2 in ((256, 256), (2048, 256), (256, 2048)):
        r = ops.gemm_tn_route(14500, n1, k2, colsum=True)
        assert (r.kernel, r.bi, r.bj, r.uses_partials_ws) == (L.TN_128, 128, 128, 0) and r.nsplit > 1
    for M in (10, 256, 512):
        r = ops.gemm_tn_route(M, 256, 256, colsum=True)
        assert (r.kernel, r.nsplit) == (L.TN_SMALL, 1)
    assert ops.gemm_tn_route(513, 256, 256).kernel == L.TN_128
    assert ops.gemm_tn_route(256, 256, 256, row_scale=True).kernel == L.TN_128             # no row scale in the short kernel


def test_knobs_move_the_routes():
    """Each selection knob the GPU tests rely on changes the route it is meant to change."""
    with L.knobs(FOD_NT_BIG=2, FOD_NT_SMALL=0):
        assert _nt(ops.gemm_nt_route(300, 128, 128)) == (L.NT_BIG, 128, 1)
        with L.knobs(FOD_NT_BIG256=2):
            assert _nt(ops.gemm_nt_route(300, 256, 128)) == (L.NT_BIG, 256, 1)
    with L.knobs(FOD_NT_BIG=0):
        assert ops.conv2d_route(L.CONV_FWD, _conv(256, 256, 3, 57, 100)).kernel == L.NT_128
    with L.knobs(FOD_NT_SPLITK=0):
        assert ops.gemm_nt_route(256, 256, 2048).ksplit == 1
    with L.knobs(FOD_TN_BIG=2, FOD_TN_SMALL=0, FOD_TN_BIG_SPLITS=3):
        r = ops.gemm_tn_route(130, 256, 128, colsum=True)
        assert (r.kernel, r.nsplit, r.uses_partials_ws) == (L.TN_BIG, 3, 0)                # M < 8192: no workspace handed over
        with L.knobs(FOD_TN_BIG256=2):
            r = ops.gemm_tn_route(130, 256, 256)
            assert (r.kernel, r.bi, r.bj) == (L.TN_BIG, 256, 256)
    with L.knobs(FOD_TN_BIG=0):
        assert ops.conv2d_route(L.CONV_WGRAD, _conv(256, 256, 3, 57, 100)).kernel == L.TN_128
    with L.knobs(FOD_TN_BIG_DENSE=1):
        r = ops.gemm_tn_route(14500, 2048, 256)
        assert r.kernel == L.TN_BIG and r.uses_partials_ws
        with L.knobs(FOD_TN_WS=0):
            assert not ops.gemm_tn_route(14500, 2048, 256).uses_partials_ws
        with L.knobs(FOD_TN_XCD=0):
            assert not ops.gemm_tn_route(14500, 2048, 256).xcd_order


def test_python_mirrors_agree_with_the_library():
    """ops.nt_wants_split_ws / ops.tn_may_use_partials_ws are what the wrappers decide the scratch by: over M = 1 .. 20 000
    and the widths and depths the model uses, split-K scratch is attached exactly where the library would use it, and
    no launch that would take partial tiles is left without a workspace."""
    dims = (64, 128, 256, 512, 1024, 2048)
    ms = sorted(set(range(1, 600, 7)) | set(range(600, 20001, 97)) | {64, 256, 512, 513, 2900, 4096, 8191, 8192, 14500, 20000})
    full = L.LIB.fod_workspace_bytes(L.WS_TN_PARTIALS)
    checked = split = partials = 0
    for M in ms:
        for N in dims:
            for K in dims:
                r = ops.gemm_nt_route(M, N, K)
                assert bool(r.wants_split_ws) == ops.nt_wants_split_ws(M, N, K), (M, N, K)
                assert (r.ksplit > 1) == bool(r.wants_split_ws), (M, N, K)                 # ... and handed over, it is used
                split += r.ksplit > 1
                for dense in (False, True):
                    with L.knobs(FOD_TN_BIG_DENSE=int(dense)):
                        t = L.TnRoute()                    # with a workspace, whatever the wrapper would do
                        ops.call("fod_gemm_tn_route", L.BF16, M, N, K, N, K, K, 0, 1, 0, full, C_addr(t))
                    if t.uses_partials_ws:
                        partials += 1
                        assert ops.tn_may_use_partials_ws(M), (M, N, K)
                checked += 1
    assert checked == len(ms) * 36 and split > 100 and partials > 1000, (checked, split, partials)
    for geom in (_conv(256, 256, 3, 57, 100), _conv(64, 64, 3, 225, 400), _conv(2048, 512, 1, 29, 50)):
        t = L.TnRoute()
        ops.call("fod_conv2d_route", L.CONV_WGRAD, L.BF16, C_addr(geom), None, 0, full, C_addr(t))
        assert not t.uses_partials_ws or ops.tn_may_use_partials_ws(geom.Nimg * geom.Ho * geom.Wo)


def C_addr(struct):
    import ctypes
    return ctypes.addressof(struct)


def test_route_queries_check_their_arguments():
    r = L.NtRoute()
    assert L.LIB.fod_gemm_nt_route(L.BF16, 250, 0, 250, 256, 64, 256, 250, None, C_addr(r)) != 0 and "multiples" in L.last_error()
    assert L.LIB.fod_gemm_nt_route(L.BF16, 256, 0, 256, 256, 64, 256, 256, None, None) != 0
    assert L.LIB.fod_conv2d_route(7, L.BF16, C_addr(_conv(64, 64, 3, 8, 8)), None, 0, 0, C_addr(r)) != 0
    a, shp = L.AttnRoute(), L.AttnShape(1, 2, 64, 64, 4096, 64, 4096, 64, 4096, 64, 4096, 64, 0.1)
    assert L.LIB.fod_attn_route(L.BF16, 1, C_addr(shp), C_addr(a)) == 0
    assert L.LIB.fod_attn_route(L.BF16, 3, C_addr(shp), C_addr(a)) != 0 and L.LIB.fod_attn_route(7, 1, C_addr(shp), C_addr(a)) != 0
    assert L.LIB.fod_attn_route(L.BF16, 1, None, C_addr(a)) != 0 and L.LIB.fod_attn_route(L.BF16, 1, C_addr(shp), None) != 0
    shp.q_token_stride = 60
    assert L.LIB.fod_attn_route(L.BF16, 1, C_addr(shp), C_addr(a)) != 0 and "multiples of 8" in L.last_error()


# ---- the attention route (fod_attn_route) -------------------------------------------------------------------------------
def _attn(r):
    return (r.fwd, r.dq, r.dkv, r.fwd_waves, r.key_split)


PLAIN, LDS, PF = L.ATTN_PLAIN, L.ATTN_LDS, L.ATTN_PREFETCH
ATTN_GRID = [(B, H, Tq, S) for B in (1, 2) for H in (1, 8) for Tq in (1, 33, 128, 512, 513, 1450)
             for S in (1, 127, 128, 255, 256, 1450)]


def test_attention_default_routes():
    """DESIGN.md §3 / launch_all in a table.  bf16 with Tq > 512 or S < 128: the three LDS kernels, eight-wave forward;
    Tq <= 512 and S >= 128: the keys split over a block's waves, prefetching dK/dV; f32: the plain kernels everywhere;
    dropout: never the LDS kernels.  Keys are split across blocks only for Tq <= 512 and S >= 256, in whole 128-key
    tiles, at most 8 ways, and only while the launch stays within one round of 256 blocks."""
    for B, H, Tq, S in ATTN_GRID:
        split = int(Tq <= 512 and S >= 128)
        for parts in (1, 2):
            r = ops.attn_route(B, H, Tq, S, parts)
            assert _attn(r) == ((PLAIN, PLAIN, PF, 4, 1) if split else (LDS, LDS, LDS, 8, 0)), (B, H, Tq, S)
            assert _attn(ops.attn_route(B, H, Tq, S, parts, torch.float32)) == (PLAIN, PLAIN, PLAIN, 4, split)
            assert _attn(ops.attn_route(B, H, Tq, S, parts, drop_p=0.1)) == (PLAIN, PLAIN, PF, 4, split)
            assert _attn(ops.attn_route(B, H, Tq, S, parts, torch.float32, drop_p=0.1)) == (PLAIN, PLAIN, PLAIN, 4, split)
            for q in (r, ops.attn_route(B, H, Tq, S, parts, torch.float32), ops.attn_route(B, H, Tq, S, parts, drop_p=0.1)):
                assert (q.ksplit, q.kchunk) == (r.ksplit, r.kchunk)        # the split across blocks is the shape's alone
            tiles = B * H * ((Tq + 31) // 32)
            if Tq > 512 or S < 256:
                assert (r.ksplit, r.kchunk) == (1, S)
            else:
                assert 1 <= r.ksplit <= min(8, S // 128) and r.ksplit * tiles <= max(256, tiles)
                assert r.kchunk % 128 == 0 or r.ksplit == 1
                assert (r.ksplit - 1) * r.kchunk < S <= r.ksplit * r.kchunk
    r = ops.attn_route(2, 8, 128, 1450, 2)                                 # the decoder's cross-attention
    assert (r.ksplit, r.kchunk) == (4, 384)


def test_attention_scratch_decides_the_split_across_blocks():
    """Without the caller's scratch (either pointer NULL) the keys are not split across blocks; the query looks at the
    pointers for NULL / non-NULL only (the addresses handed over here are not mapped)."""
    E = 32
    for ws, tk, want in ((None, None, 1), (4096, None, 1), (None, 4096, 1), (4096, 8, 8)):
        shp = L.AttnShape(1, 1, 33, 2000, 33 * E, E, 2000 * E, E, 2000 * E, E, 33 * E, E, 0.1, 0, 0, 0, 0, 0.0, 0, None, ws, tk)
        r = L.AttnRoute()
        ops.call("fod_attn_route", L.BF16, 1, C_addr(shp), C_addr(r))
        assert r.ksplit == want and r.key_split == 1


def test_attention_knobs_move_the_routes():
    """FOD_ATTN_LDS / FOD_ATTN_PF as csrc/knobs.h describes them: 0 = no LDS-staged kernels (forward, dq and dK/dV
    together), 4 = the four-wave forward, 8 = the eight-wave one; FOD_ATTN_PF=0 = no prefetching dK/dV kernel.  Neither
    touches a launch the other family owns, f32, or the split across blocks."""
    long_, few = (1, 2, 600, 333), (1, 2, 128, 300)
    assert (L.knob("FOD_ATTN_LDS"), L.knob("FOD_ATTN_PF")) == ("8", "1")
    base_few = ops.attn_route(*few)
    with L.knobs(FOD_ATTN_LDS=0):
        assert _attn(ops.attn_route(*long_)) == (PLAIN, PLAIN, PF, 4, 0)
        assert _attn(ops.attn_route(*few)) == _attn(base_few)
        with L.knobs(FOD_ATTN_PF=0):
            assert _attn(ops.attn_route(*long_)) == (PLAIN, PLAIN, PLAIN, 4, 0)
    with L.knobs(FOD_ATTN_LDS=4):
        assert _attn(ops.attn_route(*long_)) == (LDS, LDS, LDS, 4, 0)
        assert _attn(ops.attn_route(*long_, drop_p=0.1)) == (PLAIN, PLAIN, PF, 4, 0)
    with L.knobs(FOD_ATTN_LDS=8):
        assert _attn(ops.attn_route(*long_)) == (LDS, LDS, LDS, 8, 0)
    with L.knobs(FOD_ATTN_PF=0):
        assert _attn(ops.attn_route(*long_)) == (LDS, LDS, LDS, 8, 0)
        assert _attn(ops.attn_route(*few)) == (PLAIN, PLAIN, PLAIN, 4, 1)
        assert _attn(ops.attn_route(*long_, drop_p=0.1)) == (PLAIN, PLAIN, PLAIN, 4, 0)
        r = ops.attn_route(*few)
        assert (r.ksplit, r.kchunk) == (base_few.ksplit, base_few.kchunk) and base_few.ksplit > 1
    for knobs in (dict(FOD_ATTN_LDS=0), dict(FOD_ATTN_LDS=4), dict(FOD_ATTN_PF=0)):
        with L.knobs(**knobs):
            for shape in (long_, few):
                assert _attn(ops.attn_route(*shape, dtype=torch.float32))[:3] == (PLAIN, PLAIN, PLAIN)


def test_python_mirror_of_the_attention_scratch_agrees_with_the_library():
    """ops.attn_wants_split_ws decides whether _attn_shape hands the key-split scratch over: the library never splits
    across blocks where the wrapper would not have attached it."""
    E = 32
    for B, H, Tq, S in ATTN_GRID:
        shp = L.AttnShape(B, H, Tq, S, Tq * H * E, H * E, S * H * E, H * E, S * H * E, H * E, Tq * H * E, H * E, 0.1, 0, 0, 0,
                          0, 0.0, 0, None, 16, 16)
        r = L.AttnRoute()
        ops.call("fod_attn_route", L.BF16, 1, C_addr(shp), C_addr(r))
        assert r.ksplit == 1 or ops.attn_wants_split_ws(Tq, S), (B, H, Tq, S)
        assert r.ksplit == ops.attn_route(B, H, Tq, S).ksplit


# ---- the table of variant cases (tests/variant_cases.py) ------------------------------------------------------------------
@pytest.mark.parametrize("family", sorted({c.family for c in V.CASES}))
def test_variant_table_routes(family):
    """Every case of tests/test_variants_gpu.py takes, under its knobs and mode, the kernel the table says: held against
    the library here, before any GPU visit."""
    mine = V.cases(family)
    assert mine
    for c in mine:
        assert V.route_mismatches(c) == [], V.case_id(c)
        for name, value in c.knobs.items():                  # ... and the knobs are values the library takes
            with L.knobs(**{name: value}):
                assert L.knob(name) == str(value)
    assert len({V.case_id(c) for c in mine}) == len(mine)


def test_variant_table_census():
    """The table as a whole reaches every selectable variant: a variant cannot drop out when a threshold moves, because
    the route of each case is the library's (test_variant_table_routes) and the set of routes is counted here."""
    def routes(family, *fields, **where):
        return {tuple(c.expect[f] for f in fields) for c in V.cases(family, **where)}

    # NT_128 with the 128-wide tile: dense with the vector and the scalar epilogue, conv forward, dgrad, stride-2 dgrad
    for dt in V.BOTH:
        for where in (dict(call="gemm_nt", epilogue="vector"), dict(call="gemm_nt", epilogue="scalar"), dict(call="conv_fwd"),
                      dict(call="conv_dgrad", stride=1), dict(call="conv_dgrad", stride=2)):
            assert routes("nt128", "kernel", "tile_n", dtype=dt, **where) == {(L.NT_128, 128)}, (dt, where)
        assert any(c.shape[1] % 128 and c.shape[1] % 4 == 0 for c in V.cases("nt128", call="gemm_nt", dtype=dt))   # ragged last tile
        assert all(c.shape[1] % 4 for c in V.cases("nt128", epilogue="scalar"))
        assert V.cases("nt128", dtype=dt, full_epilogue=True)
    assert routes("nt_splitk", "kernel") == {(L.NT_SMALL,)}
    assert {k for (k,) in routes("nt_splitk", "ksplit")} >= {1, 2, 3, 4, 8}
    assert any(c.shape[2] % (256 * c.expect["ksplit"]) for c in V.cases("nt_splitk"))          # K chunks that do not divide K
    assert routes("nt_big", "kernel", "stages", "interleave") == {(L.NT_BIG, 3, 1), (L.NT_BIG, 3, 0), (L.NT_BIG, 2, 0), (L.NT_BIG, 2, 1)}
    for call in ("gemm_nt", "conv_fwd", "conv_dgrad"):
        assert routes("nt_big", "stages", "interleave", call=call) >= {(3, 0), (2, 1)}
    # TN_128: both block orders, an XCD-ordered launch whose split count is no multiple of 8, plain and deterministic
    for dt in V.BOTH:
        assert routes("tn128", "kernel", "xcd_order", dtype=dt) == {(L.TN_128, 0), (L.TN_128, 1)}
        ragged = [c for c in V.cases("tn128", dtype=dt) if c.expect["xcd_order"] and c.expect["nsplit"] % 8]
        assert {bool(c.extra.get("det")) for c in ragged} == {False, True}
        assert {23, 15} <= {c.expect["nsplit"] for c in ragged}
    # TN_BIG with several M-splits: partial tiles and atomics, dense and conv, the square tile, deterministic
    big = V.cases("tn_big")
    assert all(c.expect["kernel"] == L.TN_BIG and c.expect["nsplit"] > 1 for c in big)
    for call in ("gemm_tn", "conv_wgrad"):
        assert routes("tn_big", "uses_partials_ws", call=call) == {(0,), (1,)}
    assert any((c.expect.get("bi"), c.expect.get("bj")) == (256, 256) and c.expect["uses_partials_ws"] for c in big)
    assert any(c.extra.get("det") for c in big)
    assert any(c.shape[1] % 128 and c.shape[2] % 128 for c in V.cases("tn_big", call="gemm_tn"))     # ragged N1 and K2
    # layer norm: every width at the four row counts, the group knob at the many-row ones
    for dt in V.BOTH:
        seen = {(c.shape, c.knobs.get("FOD_LN_BWD_GROUPS")) for c in V.cases("layernorm", dtype=dt)}
        want = {((rows, D), g) for D in range(64, 513, 64) for rows in (37, 8191) for g in (None,)}
        want |= {((rows, D), g) for D in range(64, 513, 64) for rows in (8192, 8200) for g in (1, 4, 16)}
        assert seen == want
    # attention: the six (forward, dq, dK/dV) families and the split across blocks
    fams = set()
    for family in ("attn_family", "attn_ksplit", "attn_strided"):
        for c in V.cases(family, dtype="bf16"):
            e = c.expect
            fwd = "lds%d" % e["fwd_waves"] if e["fwd"] == LDS else "split" if e["key_split"] else "plain"
            dq = "lds" if e["dq"] == LDS else "split" if e["key_split"] else "plain"
            fams.add((fwd, dq, {PLAIN: "plain", LDS: "lds", PF: "prefetch"}[e["dkv"]]))
    assert fams == {("lds8", "lds", "lds"), ("lds4", "lds", "lds"), ("plain", "plain", "prefetch"), ("plain", "plain", "plain"),
                    ("split", "split", "prefetch"), ("split", "split", "plain")}
    drop = {(c.expect["key_split"], c.expect["dkv"]) for c in V.cases("attn_family") if c.extra.get("drop")}
    assert drop == {(0, PLAIN), (1, PLAIN)}
    for dt in V.BOTH:
        assert {k for (k,) in routes("attn_ksplit", "ksplit", dtype=dt)} >= {1, 2, 3, 4, 8}
    assert {(c.expect["fwd"], c.expect["key_split"], c.expect["ksplit"] > 1) for c in V.cases("attn_strided")} == \
        {(LDS, 0, False), (PLAIN, 1, True), (PLAIN, 0, False)}
    assert {c.expect["fwd_waves"] for c in V.cases("attn_extreme")} == {4, 8} and V.cases("attn_saturated")
    # no route query sees these two knobs: the cases exist, and the knob reads back (test_variant_table_routes)
    assert len(V.cases("fp8_stage2")) == 8 and all(c.knobs == dict(FOD_FP8_STAGE=2) for c in V.cases("fp8_stage2"))
