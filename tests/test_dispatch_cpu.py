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
