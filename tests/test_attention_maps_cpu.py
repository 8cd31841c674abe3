"""Attention maps without a GPU: the two entry points in the header and the binding, every argument check (they return
before a launch), the frame map of both memory modes, the CPU form of the overlay against an independent numpy
restatement, the colour table's rule, and the limits recorded in tests/attention_map_cases.py against the measurement."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import attention_map_cases as AC
from future_od.models import paper
from future_od.models.transformer import AttentionTap, SlotToImageAttention
from future_od.native import abi
from future_od.native import lib as L
from future_od.utils import visualization as V

I, P, LONG, FL = "int", "pointer", "long", "float"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_read_from_the_extension_header():
    assert abi.EXT_PROTOTYPES["fod_attn_maps"] == (I, [I, I, P, P, I, P, P, P])
    assert abi.EXT_PROTOTYPES["fod_render_attention"] == (
        I, [P, I, P, I, I, I, I, I, LONG, LONG, P, P, P, P, I, I, LONG, LONG, P, P, FL, FL, P])
    for name in ("fod_attn_maps", "fod_render_attention"):
        assert name not in abi.PROTOTYPES
        assert name in L.EXT_SIGNATURES and name in L._ENTRY and name not in L.SIGNATURES and name not in L.FAST
        fn = getattr(L.LIB, name)
        assert fn.restype is abi.CTYPE[I] and list(fn.argtypes) == [abi.CTYPE[k] for k in abi.EXT_PROTOTYPES[name][1]]


def test_abi_version_counts_the_new_entries():
    with open(os.path.join(ROOT, "include", "fod.h")) as f:
        hdr = f.read()
    assert int(re.search(r"#define FOD_ABI_VERSION (\d+)", hdr).group(1)) == L.ABI_VERSION == L.LIB.fod_abi_version() >= 14


# ---- argument checks: none of these calls reaches a kernel, so they run without a device -------------------------------
FAKE = 0x10000                                      # a non-NULL, 16-byte aligned address that is never read


def _shape(B=2, H=8, Tq=33, S=130, drop_p=0.0, **kw):
    E = 32 * H
    s = L.AttnShape(B, H, Tq, S, Tq * E, E, S * E, E, 0, 0, 0, 0, 0.125, 0, E, 0, 0, float(drop_p), 0, None, None, None, 0.0)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _maps_rc(dtype=L.BF16, njobs=2, ptrs="auto", query_idx=FAKE, Q=33, out=FAKE, shape="auto", jobs=None):
    if jobs is None:
        jobs = [(FAKE, FAKE, FAKE, FAKE)] * max(min(njobs, 32), 0)
    arr = (C.c_void_p * max(4 * len(jobs), 1))()
    for i, job in enumerate(jobs):
        for k, a in enumerate(job):
            arr[4 * i + k] = a
    shp = _shape() if shape == "auto" else shape
    return L.LIB.fod_attn_maps(dtype, njobs, C.addressof(arr) if ptrs == "auto" else ptrs, query_idx, Q, out,
                               None if shp is None else C.addressof(shp), None)


MAPS_REFUSED = {
    "njobs 0": dict(njobs=0), "njobs 33": dict(njobs=33), "njobs -1": dict(njobs=-1),
    "Q 0": dict(Q=0), "Q 1025": dict(Q=1025),
    "Tq 0": dict(shape=_shape(Tq=0)), "Tq 1025": dict(shape=_shape(Tq=1025)),
    "S 0": dict(shape=_shape(S=0)), "S -3": dict(shape=_shape(S=-3)),
    "q2 without k2": dict(jobs=[(FAKE, FAKE, FAKE, None)] * 2), "k2 without q2": dict(jobs=[(FAKE, None, FAKE, FAKE)] * 2),
    "second part in one job only": dict(jobs=[(FAKE, FAKE, FAKE, FAKE), (FAKE, None, FAKE, None)]),
    "second part in the later job only": dict(jobs=[(FAKE, None, FAKE, None), (FAKE, FAKE, FAKE, FAKE)]),
    "null out": dict(out=None),
    "drop_p": dict(shape=_shape(drop_p=0.1)),
    "null q1": dict(jobs=[(None, FAKE, FAKE, FAKE)] * 2), "null k1": dict(jobs=[(FAKE, FAKE, None, FAKE)] * 2),
    "null ptrs": dict(ptrs=None), "null shape": dict(shape=None),
    "identity with Q != Tq": dict(query_idx=None, Q=32),
    "bad dtype": dict(dtype=7), "H 65": dict(shape=_shape(H=65)), "B 0": dict(shape=_shape(B=0)),
    "misaligned operand": dict(jobs=[(FAKE + 2, FAKE, FAKE, FAKE)] * 2),
    "stride not a multiple of 8": dict(shape=_shape(q_token_stride=260)),
}


@pytest.mark.parametrize("what", list(MAPS_REFUSED))
def test_attn_maps_refuses_before_any_launch(what):
    assert _maps_rc(**MAPS_REFUSED[what]) == L.ERR_ARG, what
    assert "attn_maps" in L.last_error()


def _render_rc(**kw):
    a = dict(src=FAKE, u8=0, dst=FAKE, B=2, L=3, J=3, H=7, W=9, sb=3 * 3 * 63, sl=3 * 63, frame_idx=FAKE, mean=FAKE, std=FAKE,
             maps=FAKE, h=2, w=3, mb=54, mj=6, cs=FAKE, lut=FAKE, gain=50.0, max_alpha=0.4)
    a.update(kw)
    return L.LIB.fod_render_attention(a["src"], a["u8"], a["dst"], a["B"], a["L"], a["J"], a["H"], a["W"], a["sb"], a["sl"],
                                      a["frame_idx"], a["mean"], a["std"], a["maps"], a["h"], a["w"], a["mb"], a["mj"],
                                      a["cs"], a["lut"], a["gain"], a["max_alpha"], None)


RENDER_REFUSED = {
    "null src": dict(src=None), "null dst": dict(dst=None), "null frame_idx": dict(frame_idx=None),
    "null maps": dict(maps=None), "null colour_scale": dict(cs=None), "null lut": dict(lut=None),
    "f32 without mean": dict(mean=None), "f32 without std": dict(std=None),
    "h 0": dict(h=0), "w 0": dict(w=0), "J 0": dict(J=0), "J 33": dict(J=33),
    "max_alpha below 0": dict(max_alpha=-0.01), "max_alpha above 1": dict(max_alpha=1.5), "max_alpha NaN": dict(max_alpha=float("nan")),
    "gain inf": dict(gain=float("inf")), "gain NaN": dict(gain=float("nan")),
    "frame stride": dict(sl=3 * 63 - 1), "negative map stride": dict(mj=-6), "B 0": dict(B=0),
}


@pytest.mark.parametrize("what", list(RENDER_REFUSED))
def test_render_attention_refuses_before_any_launch(what):
    assert _render_rc(**RENDER_REFUSED[what]) == L.ERR_ARG, what
    assert "render_attention" in L.last_error()


# ---- the model's side ---------------------------------------------------------------------------------------------------
def _core(mode, num_images):
    return SimpleNamespace(detector=SimpleNamespace(image_memory_mode=mode, num_images=num_images))


def test_frame_map_of_both_memory_modes():
    frames = paper.FuturePredCore._memory_frames
    # one at a time: image j is clip frame past - 1 - j, as many as there are blocks and encoded frames
    assert frames(_core("attend one at a time", 3), 5, 3) == ([4, 3, 2], 1)
    assert frames(_core("attend one at a time", 5), 2, 2) == ([1, 0], 1)
    assert frames(_core("attend one at a time", 2), 4, 4) == ([3, 2], 1)          # slot states: every frame is encoded
    assert frames(_core("attend one at a time", 1), 1, 1) == ([0], 1)
    # all at once: ONE memory, its keys are the encoded frames oldest first
    assert frames(_core("attend all at once", 1), 4, 4) == ([0, 1, 2, 3], 4)
    assert frames(_core("attend all at once", 1), 1, 1) == ([0], 1)


def test_f2f_core_has_no_per_frame_memory():
    f2f = paper.JointEncoderF2F.__new__(paper.JointEncoderF2F)
    core = SimpleNamespace(attention_tap=AttentionTap(), joint_encoder=f2f)
    with pytest.raises(ValueError, match="JointEncoderF2F"):
        paper.FuturePredCore.forward(core, torch.zeros(1, 3, 3, 8, 8))


def test_tap_is_off_by_default_and_keeps_the_last_pass():
    block = SlotToImageAttention(64, 2, 0.0)
    assert block.attention_tap is None and block.store_attention is False and paper.FuturePredCore.attention_tap is None
    tap = AttentionTap()
    tap("qc", "qs", "side", 5, 0)
    tap("qc", "qs", "side", 5, 1)
    tap("qc2", "qs2", "side2", 5, 0)
    assert tap.blocks == {0: ("qc2", "qs2", "side2", 5, 0), 1: ("qc", "qs", "side", 5, 1)}
    with pytest.raises(ValueError):
        AttentionTap().maps(8)


def test_head_mean_weights_is_the_float64_reference_on_cpu_tensors():
    """The CPU form of stored_attention, against the cases' reference (one block, all queries)."""
    from future_od.models.transformer import _head_mean_weights
    case = AC.BY_NAME["f32 dense identity"]
    jobs, scale, _ = AC.build(case)
    q1, q2, k1, k2 = jobs[0]
    ref, _ = AC.reference(jobs[:1], scale, case.H)
    got = _head_mean_weights(q1, k1, q2, k2.unsqueeze(0).expand(case.B, -1, -1), case.H)
    assert AC.distance(got, ref[:, :, 0], torch.ones(case.B, case.Tq, dtype=torch.bool)) <= 3 * AC.D32[case.name] + 1e-6


# ---- the overlay --------------------------------------------------------------------------------------------------------
def test_colour_table_rule():
    lut = V.ATTENTION_LUT
    assert lut.dtype == torch.uint8 and tuple(lut.shape) == (256, 3)
    assert np.array_equal(lut.numpy(), AC.LUT)
    assert lut[0].tolist() == [0, 0, 255] and lut[255].tolist() == [255, 0, 0]
    assert lut[127].tolist() == [254, 254, 255] and lut[128].tolist() == [255, 254, 254]
    v = lut.to(torch.int32)
    assert bool((v[1:128, 0] - v[:127, 0] == 2).all()) and bool((v[:128, 0] == v[:128, 1]).all()) and bool((v[:128, 2] == 255).all())
    assert bool((v[128:-1, 1] - v[129:, 1] == 2).all()) and bool((v[128:, 1] == v[128:, 2]).all()) and bool((v[128:, 0] == 255).all())


OVERLAY = AC.overlay_cases()


@pytest.mark.parametrize("case", OVERLAY, ids=[c["name"] for c in OVERLAY])
def test_cpu_render_attention_gives_the_restated_bytes(case):
    slot = case["slot"] if isinstance(case["slot"], int) else torch.from_numpy(case["slot"])
    got = V.render_attention(torch.from_numpy(case["video"]), torch.from_numpy(case["attention"]),
                             torch.tensor(case["frames"], dtype=torch.int32), slot, case["gain"], case["max_alpha"])
    want = AC.overlay_expected(case)
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    assert np.array_equal(got.numpy(), want), int((got.numpy() != want).sum())


def test_overlay_cases_show_something():
    """The comparison above is not between two plain frames: the overlay changes most pixels, and with gain 0 or
    max_alpha 0 none."""
    for case in OVERLAY:
        want = AC.overlay_expected(case)
        L_ = case["video"].shape[1]
        plain = np.stack([[AC.RC.background(case["video"][b, min(max(f + L_ if f < 0 else f, 0), L_ - 1)])
                           for f in case["frames"]] for b in range(case["video"].shape[0])])
        changed = float((want != plain).any(-1).mean())
        if case["gain"] == 0.0 or case["max_alpha"] == 0.0:
            assert changed == 0.0, case["name"]
        else:
            assert changed > 0.5, (case["name"], changed)


def test_render_attention_refuses_what_the_kernel_refuses():
    video, att = torch.zeros(1, 1, 3, 4, 4), torch.zeros(1, 1, 1, 2, 2)
    with pytest.raises(ValueError):
        V.render_attention(video, att, [0], 0, max_alpha=1.5)
    with pytest.raises(ValueError):
        V.render_attention(video[0], att, [0], 0)
    with pytest.raises(ValueError):
        V.render_attention(video, att[0], [0], 0)


# ---- the recorded limits ------------------------------------------------------------------------------------------------
def test_every_case_has_a_recorded_distance_and_the_edges_are_there():
    assert set(AC.D32) == set(AC.BY_NAME) and AC.MEASURED_FACTOR == 3.0 and AC.ROUNDINGS == 8 * 2.0 ** -24
    cs = AC.MAP_CASES
    assert {1, 63, 64, 65, 130} <= {c.S for c in cs} and any(c.S >= 512 for c in cs)
    assert {1, 31, 32, 33} <= {c.Q for c in cs if c.table} and {1, 31, 32, 33} <= {c.Q for c in cs if not c.table}
    assert {1, 2} == {c.parts for c in cs} and {True, False} == {c.k2_per_batch for c in cs} == {c.strided for c in cs}
    assert {1, 2, 5, 32} <= {c.njobs for c in cs} and {1, 8} <= {c.H for c in cs} and {1, 2} <= {c.B for c in cs}
    assert {("bf16", g) for g in (1.0, 4.0, 12.0)} | {("f32", g) for g in (1.0, 4.0, 12.0)} <= {(c.dtype, c.gain) for c in cs}
    idx = AC.query_table(2, 33, 33, 4)
    assert bool((idx == -1).any()) and bool((idx == 33).any()) and len(set(idx[0].tolist())) < 33


@pytest.mark.parametrize("name", list(AC.BY_NAME))
def test_recorded_distance_is_current(name):
    """Within a factor of two either way (test_criterion_limits_cpu.py): the figure is a maximum that hangs on single
    roundings of exp, so another libm may move it a little; a changed case moves it by more and is measured again."""
    now, recorded = AC.measure_d32(AC.BY_NAME[name]), AC.D32[name]
    assert 0.5 * recorded <= now <= 2.0 * recorded, (name, now, recorded)


def test_gain_12_is_a_one_hot_softmax_with_scores_of_several_thousand():
    case = AC.BY_NAME["gain12"]
    jobs, scale, idx = AC.build(case)
    ref, A = AC.reference(jobs, scale, case.H, idx)
    assert A > 500.0                    # the exponent argument; the raw scores of one part are several thousand
    part = (jobs[0][0].double().view(case.B, case.Tq, case.H, 32).transpose(1, 2)
            @ jobs[0][2].double().view(case.B, case.S, case.H, 32).transpose(1, 2).transpose(-1, -2))
    assert float(part.abs().max()) > 2000.0
    valid = AC.valid_rows(idx, case.B, case.Q, case.Tq)
    assert float(ref.amax(-1)[valid].min()) > 1 / 16 and bool((ref.sum(-1)[valid] - 1).abs().max() < 1e-12)
    assert bool((ref[~valid] == 0).all())
