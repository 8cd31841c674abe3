"""future_od/native/detect.py owns the detection-row operations, ops.py forwards their old names: identity of the
forwarded names, both import orders in fresh processes, launches that still pass through `ops.call`, the one operand
checker's message text (written out here as the wrappers produced it before they shared a checker), and the row limit
against csrc/det_rows.h.  No GPU."""
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "future-object-detection_amd")

MOVED = ("post_proc", "detect_select", "detect_nms", "od_map", "detect_od_map", "track_update", "AP_HIST_BINS",
         "AP_HIST_POINTS", "ap_hist_keys", "ap_hist_state", "ap_hist_accum", "ap_hist_finalize")


def test_ops_forwards_every_moved_name_to_the_same_object():
    from future_od.native import detect, ops
    for n in MOVED:
        assert getattr(ops, n) is getattr(detect, n), n
    assert ops._IN_DETECT == MOVED
    with pytest.raises(AttributeError, match="no_such_name"):
        ops.no_such_name
    for n in ("tracker_cost", "tracker_extrapolate", "set_loss_fwd", "call", "stream"):     # these did not move
        assert n in vars(ops) and n not in vars(detect), n


@pytest.mark.parametrize("first", ["detect", "ops"])
def test_either_module_may_be_imported_first(first):
    """Two overlapping boxes of one class, the second a little smaller: NMS at 0.5 keeps row 0 only."""
    code = ("import sys; sys.path[:0] = [sys.argv[1], sys.argv[2]]\n"
            f"import future_od.native.{first}\n"
            "import torch\nfrom future_od.native import ops\n"
            "i32 = torch.int32\n"
            "out = ops.detect_nms(torch.tensor([[0.9, 0.8]]), torch.zeros(1, 2, dtype=i32),\n"
            "                     torch.tensor([[[0., 0., 10., 10.], [1., 1., 10., 10.]]]), torch.tensor([[4, 7]], dtype=i32),\n"
            "                     torch.tensor([2], dtype=i32))\n"
            "print('KEPT', int(out[4][0]), out[3][0].tolist(), out[5][0].tolist())\n")
    r = subprocess.run([sys.executable, "-c", code, ROOT, PKG], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "KEPT 1 [4, -1] [0, -1]" in r.stdout, (r.stdout, r.stderr[-2000:])


def test_a_launch_goes_through_ops_call(monkeypatch):
    """tools/grad_fanout.py and tools/tn_direct_sites.py count launches by replacing `ops.call`."""
    from future_od.native import detect, ops
    seen = []
    monkeypatch.setattr(ops, "call", lambda name, *a, **k: seen.append((name, a)))
    monkeypatch.setattr(ops, "stream", lambda: 0)
    monkeypatch.setattr(detect, "_chk", lambda t, *a: t)                # (the device test: these are host tensors)
    logits, boxes = torch.zeros(2, 3, 5), torch.zeros(2, 3, 4)
    scores, boxes_px = detect.post_proc(logits, boxes, 96, 128)
    assert [name for name, _ in seen] == ["fod_post_proc"]
    assert seen[0][1] == (logits.data_ptr(), boxes.data_ptr(), scores.data_ptr(), boxes_px.data_ptr(), 6, 5, 96.0, 128.0, 0)
    assert scores.shape == (2, 3, 6) and boxes_px.shape == (2, 3, 4)


def _rows():
    i32 = torch.int32
    return (torch.zeros(1, 2), torch.zeros(1, 2, dtype=i32), torch.zeros(1, 2, 4), torch.zeros(1, 2, dtype=i32),
            torch.tensor([2], dtype=i32))


def test_the_checker_keeps_the_message_text():
    from future_od.native import detect
    from future_od.native import lib as L
    s, l, b, q, c = _rows()
    od = (torch.zeros(1, 2, 3), torch.zeros(1, 2, 3, dtype=torch.uint8), torch.zeros(2, 4, 3, dtype=torch.uint8),
          torch.zeros(2, 4, dtype=torch.int64))
    state = detect.ap_hist_state(1, 2, "cpu")
    cases = (
        # a wrong dtype
        (lambda: detect.detect_nms(s, l.long(), b, q, c),
         "detect_nms: contiguous labels torch.int32 [1, 2] on cpu expected, got torch.int64 (1, 2) strides (2, 1) on cpu"),
        # a wrong shape, in an `out` slot
        (lambda: detect.detect_nms(s, l, b, q, c, out=(s, l, b, q, c, torch.zeros(1, 3, dtype=torch.int32))),
         "detect_nms: contiguous out source torch.int32 [1, 2] on cpu expected, got torch.int32 (1, 3) strides (3, 1) on cpu"),
        # not contiguous
        (lambda: detect.detect_nms(s, l, torch.zeros(1, 4, 2).transpose(1, 2), q, c),
         "detect_nms: contiguous boxes torch.float32 [1, 2, 4] on cpu expected, got torch.float32 (1, 2, 4) strides "
         "(8, 1, 2) on cpu"),
        # a bool | uint8 slot names bool
        (lambda: detect.ap_hist_accum((od[0], od[1].int(), od[2], od[3]), state),
         "ap_hist_accum: contiguous is_positive torch.bool [1, 2, 3] on cpu expected, got torch.int32 (1, 2, 3) strides "
         "(6, 3, 1) on cpu"),
        (lambda: detect.detect_od_map(s, l, b, q, c, torch.zeros(1, 3, 4), torch.zeros(1, 3, dtype=torch.int64),
                                      torch.zeros(1, 3, dtype=torch.int64), (96, 128), 2, T=1,
                                      out=(torch.zeros(1, 3, 2), torch.zeros(1, 3, 2), torch.zeros(3, 4, 2, dtype=torch.bool),
                                           torch.zeros(3, 4, dtype=torch.int64))),
         "detect_od_map: contiguous out is_positive torch.bool [1, 3, 2] on cpu expected, got torch.float32 (1, 3, 2) "
         "strides (6, 2, 1) on cpu"),
        # the streaming state
        (lambda: detect.ap_hist_finalize((state[0], state[1][:, :, :5], state[2])),
         "ap_hist_finalize: contiguous state hist_seen torch.int32 [2, 4, 16257] on cpu expected, got torch.int32 (2, 4, 5) "
         "strides (65028, 16257, 1) on cpu"),
    )
    for bad, text in cases:
        with pytest.raises(L.FodError) as e:
            bad()
        assert str(e.value) == text
    detect.ap_hist_accum(od, state)                                     # uint8 flags pass, and so do bool ones
    detect.ap_hist_accum((od[0], od[1].bool(), od[2].bool(), od[3]), state)
    # None is a slot that is not wanted (track_update's `slot`): skipped, the others are still checked
    spec = (("track", torch.int32, (1, 2)), ("hits", torch.int32, (1, 2)), ("slot", torch.int32, (1, 2)))
    detect._expect("track_update", (l, q, None), spec, l.device, "out ")
    with pytest.raises(L.FodError) as e:
        detect._expect("track_update", (l, s, None), spec, l.device, "out ")
    assert str(e.value) == ("track_update: contiguous out hits torch.int32 [1, 2] on cpu expected, got torch.float32 (1, 2) "
                            "strides (2, 1) on cpu")


def test_the_row_limit_is_the_kernels():
    from future_od.native import detect
    from future_od.native import lib as L
    hdr = open(os.path.join(PKG, "csrc", "det_rows.h")).read()
    assert int(re.search(r"constexpr int ROWS_MAX = (\d+);", hdr).group(1)) == detect.ROWS_MAX == 1024
    for name in ("detect_nms.hip", "detect_eval.hip", "track.hip"):
        assert '#include "det_rows.h"' in open(os.path.join(PKG, "csrc", name)).read(), name
    l = torch.zeros(1, 1025, dtype=torch.int32)
    with pytest.raises(L.FodError, match=r"K=1025 \(1\.\.1024\)"):
        detect.detect_nms(torch.zeros(1, 1025), l, torch.zeros(1, 1025, 4), l.clone(), torch.zeros(1, dtype=torch.int32))
