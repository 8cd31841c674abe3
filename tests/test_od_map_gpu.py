"""fod_od_map against oracle/od_map.prepare_od_map_stuffs run live on the CPU, all four outputs exactly equal, at what the
three g9 fixtures do not reach: fewer than 50 predictions, more than 64 annotations, tied scores (the kernel ranks ties by
ascending index, the oracle sorts stably), annotations that tie in IoU, IoUs exactly on a threshold and areas exactly on a
size delimiter.  B <= 2, C1 <= 4: the oracle is pure-Python loops."""
import functools
import zlib

import numpy as np
import pytest
import torch

from oracle import od_map as OM

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from future_od.native import ops

DEV = "cuda:0"
IMSIZE = (384, 512)          # (H, W): both size delimiters are exact, 128 and 4096 px^2
# name: (B, M, N, C1).  K = min(50, M): below, at and above 50; M and N off the multiples of the 64 lanes
CASES = {"m7": (1, 7, 1, 2), "m50": (2, 50, 64, 3), "m51": (2, 51, 65, 4), "m100": (1, 100, 130, 3),
         "m300": (2, 300, 130, 4)}
AREAS = {128: (8, 16), 129: (3, 43), 4096: (64, 64), 4097: (241, 17)}


def _f32(v):
    return np.asarray(v, dtype=np.float32)


def threshold_pairs():
    """[(t, pred, anno)]: integer boxes [0, 0, 10, 10 + t] in [0, 0, 10, 20] have IoU (10 + t) / 20; kept where the oracle's
    float32 IoU IS the oracle's float32 threshold, so `>=` decides at equality."""
    thr = torch.arange(0.50, 1.00, 0.05).numpy()
    out = []
    for t in range(len(thr)):
        pred, anno = _f32([0, 0, 10, 10 + t]), _f32([0, 0, 10, 20])
        if OM._iou(pred, anno) == thr[t]:
            out.append((t, pred, anno))
    assert len(out) >= 3 and out[0][0] == 0, [t for t, _, _ in out]
    return out


def _specials():
    """[(pred box, anno box)] in the strip x >= 320 that the random boxes stay out of; all annotations of class 0, all
    predictions with score 1.0 in every class, listed in the order of their indices."""
    box = lambda x, y, w, h: _f32([x, y, x + w, y + h])
    sp = []
    # two annotations at the same IoU from P1 (300 / 500 by symmetry): P1 claims the one with the lower index, so P2, which
    # sits exactly on that one, finds it taken and stays negative
    p1, a_lo, a_hi = box(400, 10, 20, 20), box(395, 10, 20, 20), box(405, 10, 20, 20)
    assert OM._iou(p1, a_lo) == OM._iou(p1, a_hi) >= np.float32(0.5) > OM._iou(a_lo, a_hi)
    sp += [(p1, a_lo), (a_lo.copy(), a_hi)]
    # a duplicated annotation (same box, same class): two predictions compete, the first takes the lower index
    dup = box(400, 50, 20, 20)
    sp += [(dup.copy(), dup.copy()), (box(401, 50, 20, 20), dup.copy())]
    for i, (t, pred, anno) in enumerate(threshold_pairs()):
        off = _f32([325 + 15 * (i % 5), 100 + 25 * (i // 5)] * 2)
        assert OM._iou(pred + off, anno + off) == OM._iou(pred, anno)
        sp.append((pred + off, anno + off))
    # areas exactly on and one above the delimiters, as predictions and as annotations: `<=` against `<`
    for (area, (w, h)), (x, y) in zip(AREAS.items(), ((330, 200), (345, 200), (360, 200), (250, 280))):
        b = box(x, y, w, h)
        assert (b[2] - b[0]) * (b[3] - b[1]) == np.float32(area)
        sp.append((b, b.copy()))
    return sp


@functools.lru_cache(maxsize=None)
def build(name):
    B, M, N, C1 = CASES[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    rnd = lambda *s: torch.rand(*s, generator=g)

    def boxes(n):
        x0, y0 = rnd(B, n) * 250, rnd(B, n) * 300
        return torch.stack([x0, y0, x0 + 4 + rnd(B, n) * 60, y0 + 4 + rnd(B, n) * 60], -1)

    pb, ab = boxes(M), boxes(N)
    near = torch.randint(0, M, (B, N), generator=g)                     # most annotations sit near some prediction
    ab[:, ::2] = (pb.gather(1, near[..., None].expand(-1, -1, 4)) + rnd(B, N, 4) * 6 - 3)[:, ::2]
    ab[..., 2:] = torch.maximum(ab[..., 2:], ab[..., :2] + 1)
    scores = torch.round(rnd(B, M, C1) * 8) / 8                         # multiples of 1/8: many exact ties
    if M >= 50:
        scores[:, 5:15] = 1.0                                           # a saturated sigmoid
    real = max(C1 - 2, 1)                                               # C1 >= 3: class C1 - 2 has no annotation at all
    classes = torch.randint(0, real, (B, N), generator=g)
    active = torch.zeros(B, N, dtype=torch.int64)
    active[0] = (torch.arange(N) % 3 != 1).long()                       # inactive rows between active ones
    if B > 1 and name != "m300":
        active[1] = (torch.arange(N) % 2 == 0).long()                   # (m300: the second sample has none active)
    if M >= 50 and N >= 64:
        sp = _specials()
        pidx = [M - 1 - 2 * i for i in reversed(range(len(sp)))]
        act = [n for n in range(N) if n % 3 != 1]
        aidx = [act[(i * len(act)) // len(sp)] for i in range(len(sp))]
        assert pidx[0] >= 15 and len(set(aidx)) == len(sp) and aidx == sorted(aidx)
        if N > 128:
            assert max(aidx) >= 64                                      # tied annotations in different trips of the loop
        for (p, a), pi, ai in zip(sp, pidx, aidx):
            pb[0, pi], ab[0, ai] = torch.from_numpy(p), torch.from_numpy(a)
            scores[0, pi], classes[0, ai] = 1.0, 0
    assert C1 < 3 or not bool((classes == C1 - 2).any())
    want = OM.prepare_od_map_stuffs(pb.numpy(), scores.numpy(), ab.numpy(), classes.numpy(), active.numpy(), IMSIZE)
    return (scores, pb, ab, classes, active), want


@pytest.mark.parametrize("name", list(CASES))
def test_od_map_equals_the_oracle_exactly(name):
    inputs, want = build(name)
    B, M, N, C1 = CASES[name]
    got = ops.od_map(*(t.to(DEV) for t in inputs), IMSIZE)
    K = min(50, M)
    assert got[0].shape == (10, C1, B * K) and want[0].shape == got[0].shape
    for what, a, b in zip(("confs", "is_positive", "size_categories", "num_annos"), got, want):
        np.testing.assert_array_equal(a.cpu().numpy(), b, err_msg=f"{name}: {what}")
    if M >= 50 and N >= 64:
        assert want[1][:, C1 - 1].any() and not want[1][:, C1 - 1].all()          # the case decides something
        assert (want[2][0, 1:].sum(1) > 0).all() and (want[3][0, 1:] > 0).all()    # every size category occurs
