"""Deterministic mode, the parts that need no GPU: the C ABI of the `_det` entry points (declared, exported, sized,
loud about their scratch before anything is launched), the one switch, and the bounded scratch of the long weight
gradients' deterministic plan at the headline extent."""
import ctypes
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "future-object-detection_amd")

DET_ENTRIES = ["fod_gemm_tn_acc_det", "fod_gemm_tn_multi_long_det", "fod_conv2d_wgrad_acc_det", "fod_colsum_acc_det",
               "fod_layernorm_bwd_det", "fod_linear_add_norm_bwd_det", "fod_mlp2_mul_bwd_det"]


def test_header_binding_and_library_agree_on_the_deterministic_entries():
    from future_od.native import lib as L
    hdr = open(os.path.join(ROOT, "include", "fod.h")).read()
    assert int(re.search(r"#define FOD_ABI_VERSION (\d+)", hdr).group(1)) == L.ABI_VERSION == L.LIB.fod_abi_version() >= 5
    for name in DET_ENTRIES:
        proto = re.search(r"^int " + name + r"\s*\(([^;]*)\);", hdr, flags=re.M)
        assert proto, f"{name} not declared in fod.h"
        assert "void* ws, size_t ws_bytes, fod_stream_t stream" in " ".join(proto.group(1).split()), name
        assert hasattr(L.LIB, name) and name in L.EXPORTS and (not L.FAST or name in L.FAST), name
        sig, twin = L.SIGNATURES[name], L.SIGNATURES[name[:-4]]
        assert sig[-3:] == [L._p, ctypes.c_size_t, L._p], name
        if name == "fod_gemm_tn_multi_long_det":           # + the per-job scratch offsets, their count and total
            assert sig[:4] == twin[:4]
        elif twin[-3:-1] == [L._p, ctypes.c_size_t]:        # the twin has an (optional) workspace already
            assert sig == twin
        else:                                              # same arguments, scratch in front of the stream
            assert sig == twin[:-1] + [L._p, ctypes.c_size_t, L._p], name
    assert L.LIB.fod_workspace_bytes(L.WS_DET) == 16 << 20
    assert L.LIB.fod_workspace_bytes(L.WS_TN_MULTI_DET) == 128 << 20
    assert int(re.search(r"#define FOD_TN_DET_MAX_SPLITS (\d+)", hdr).group(1)) == L.TN_DET_MAX_SPLITS
    # existing prototypes and layouts are untouched
    assert [f for f, _ in L.Epilogue._fields_][-2:] == ["split_ws", "split_tickets"]
    assert [f for f, _ in L.TnJob._fields_][-2:] == ["m_per_split", "nsplit"]


def _null_args(sig, ws, ws_bytes):
    """Arguments of a `_det` entry with every pointer NULL and every extent 0, except the scratch."""
    args = [None if t is ctypes.c_void_p else t(0) for t in sig]
    args[-3], args[-2] = ws, ctypes.c_size_t(ws_bytes)
    return args


@pytest.mark.parametrize("name", DET_ENTRIES)
def test_missing_or_small_scratch_is_refused_before_any_launch(name):
    """No GPU here: a launch would fail differently.  The error names the scratch and there is no atomic fallback."""
    from future_od.native import lib as L
    sig = L.SIGNATURES[name]
    fn = getattr(L.LIB, name)                               # ctypes (the fast-call wrappers share the library)
    buf = ctypes.create_string_buffer(64)
    addr = (ctypes.addressof(buf) + 15) // 16 * 16
    for ws, nbytes in ((None, 1 << 30), (addr, 1)):
        args = _null_args(sig, ws, nbytes)
        if name == "fod_gemm_tn_multi_long_det":
            args[6] = ctypes.c_size_t(1 << 20)              # part_floats the table needs
        rc = fn(*args)
        assert rc == 1, (name, ws, rc)                      # FOD_ERR_ARG
        assert "scratch" in L.last_error() and "no atomic fallback" in L.last_error(), L.last_error()
    with pytest.raises(L.FodError, match="scratch"):
        L.call(name, *[a.value if hasattr(a, "value") else a for a in _null_args(sig, None, 0)])


def test_one_switch():
    from future_od.native import functional as Fn
    from future_od.native import ops
    prev = Fn.is_deterministic()
    try:
        Fn.set_deterministic(True)
        assert Fn.is_deterministic() and ops.is_deterministic()
        Fn.set_deterministic(False)
        assert not Fn.is_deterministic() and not ops.is_deterministic()
    finally:
        Fn.set_deterministic(prev)
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from future_od.native import functional as Fn\nprint('MODE', int(Fn.is_deterministic()))" % (ROOT, PKG))
    for env_val, want in (("1", "MODE 1"), ("0", "MODE 0"), (None, "MODE 0")):
        env = {k: v for k, v in os.environ.items() if k != "FOD_DETERMINISTIC"}
        if env_val is not None:
            env["FOD_DETERMINISTIC"] = env_val
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and want in r.stdout, (env_val, r.stdout[-500:], r.stderr[-2000:])


def test_build_model_honours_args_deterministic():
    from future_od.models.st_detr import SpatioTemporalDETRArgs
    from future_od.native import functional as Fn
    from runs._model import build_model
    detr = SpatioTemporalDETRArgs(num_classes=8, num_queries=16, lr_backbone=1e-4, enc_layers=1, dec_layers=1,
                                  pretrained_backbone=False)
    prev = Fn.is_deterministic()
    try:
        for flag in (True, False):
            build_model(SimpleNamespace(device="cpu", distributed=False, compute_dtype="bf16", backbone="resnet18",
                                        deterministic=flag), detr)
            assert Fn.is_deterministic() is flag
        Fn.set_deterministic(True)       # absent from args: the switch stays where it is (as args.attn_dtype)
        build_model(SimpleNamespace(device="cpu", distributed=False, compute_dtype="bf16", backbone="resnet18"), detr)
        assert Fn.is_deterministic()
    finally:
        Fn.set_deterministic(prev)


def test_deterministic_long_job_plan_keeps_the_scratch_bounded_at_the_headline_extent():
    """10 frames x 1450 tokens, D = 256, FFN 2048, 6 + 6 layers, 5 images: the queued long weight gradients of a step.  The
    default plan has ~7 M-splits of 2048 rows per job and no scratch; the deterministic plan at most
    FOD_TN_DET_MAX_SPLITS longer ones, and cuts the jobs into launches that each fit fod_workspace_bytes(WS_TN_MULTI_DET)."""
    import numpy as np
    from future_od.native import lib as L
    from future_od.native import wgrad as W
    long_rows = W._WgradQueue().long_rows
    n = [0]

    def job(M, N1, K2, bias=True):
        n[0] += 1
        return W.Job(G=1000 * n[0] + 16, X=2000 * n[0] + 32, dW=3000 * n[0] + 48, colsum=4000 * n[0] + 64 if bias else 0,
                     ldg=N1, ldx=K2, ldw=K2, M=M, N1=N1, K2=K2)
    enc = [(512, 256), (256, 256), (256, 256), (2048, 256), (256, 2048)]        # q|k, v, out, the two feed-forward layers
    jobs = [job(14500, n1, k2) for _ in range(6) for n1, k2 in enc]
    jobs += [job(7250, 256, 256) for _ in range(6) for _ in range(3)]           # the decoder's memory-side projections
    jobs.append(job(14500, 256, 256, bias=False))
    cap = L.LIB.fod_workspace_bytes(L.WS_TN_MULTI_DET)
    groups = W.det_groups(jobs, long_rows)
    assert sum(len(g) for g in groups) == len(jobs) and [j for g in groups for j in g] == jobs      # queue order kept
    assert len(groups) >= 2                                  # (this extent does not fit one launch: the cut is exercised)
    size = ctypes.sizeof(L.TnJob)
    for group in groups:
        raw, off, nblocks, part_floats = W.long_table(group, long_rows, det=True)
        assert 0 < 4 * part_floats <= cap
        assert raw.size == off + 8 * nblocks + 8 * len(group)
        table = (L.TnJob * len(group)).from_buffer_copy(raw[:len(group) * size].tobytes())
        offs = raw[off + 8 * nblocks:].view(np.int64)
        at = 0
        for t, o in zip(table, offs):
            assert 1 < t.nsplit <= L.TN_DET_MAX_SPLITS and (t.nsplit - 1) * t.m_per_split < t.M <= t.nsplit * t.m_per_split
            assert o == at                                   # disjoint, back to back, in table order
            at += t.nsplit * (t.N1 * t.K2 + (t.N1 if t.colsum else 0))
        assert at == part_floats
    # the default plan is what it was
    raw, off, nblocks, _ = W.long_table(jobs[:5], long_rows)
    table = (L.TnJob * 5).from_buffer_copy(raw[:5 * size].tobytes())
    assert all(t.nsplit == 7 for t in table)
    # a job that cannot fit is refused, not run with atomics
    with pytest.raises(L.FodError, match="scratch"):
        W.det_groups([job(14500, 8192, 2048)], long_rows)
