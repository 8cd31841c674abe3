"""The cases of tests/test_criterion_gpu.py (fod_match_cost, fod_set_loss_fwd/bwd, fod_post_proc, fod_tracker_cost/extrapolate),
their float64 references and the limits the kernels are held to: ONE table, read by the GPU test and by
tests/test_criterion_limits_cpu.py, which measures the recorded yardsticks again on the CPU and checks the preconditions the
cases rely on.  Nothing here touches a device or the native library.

Inputs are built in float32 and the references read exactly those values as float64 (oracle/criterion.py and
oracle/thirdparty.py with float64 tensors, gradients from float64 autograd).  Every function that takes `dtype` gives the
reference with float64 and "the float32 oracle" -- the same arithmetic as torch evaluates it in float32 -- with float32.

Limits
  set losses and gradients: the bounds of test_matcher_and_losses (tests/test_heads_gpu.py), now against float64 (LOSS_TOL)
  match cost:               per logit band, atol = max(2e-5, 3 * COST_MEASURED[band]), rtol 1e-5 -- the existing bound or three
                            times the float32 oracle's own largest distance to float64, whichever is larger
  tracker kernels:          3 * TRACKER_MEASURED[op] on the error scaled by max(1, |ref|)
"""
import zlib
from collections import namedtuple

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

from oracle import criterion as ocrit
from oracle import stdetr as O
from oracle import thirdparty as tp

MEASURED_FACTOR = 3.0

# (atol, rtol) of test_matcher_and_losses; cardinality_error is compared exactly
LOSS_TOL = {"loss": (1e-5, 2e-5), "class_error": (1e-4, 1e-5), "dlogits": (1e-6, 1e-4), "dboxes": (1e-5, 1e-4)}
COST_TOL = (2e-5, 1e-5)

# max |float32 oracle - float64| of the match cost over all COST_CASES of a band, measured on the CPU
# (tests/test_criterion_limits_cpu.py fails when a figure is more than a factor of two from what it measures).
# The class cost holds -log(1 - p + 1e-8): near p = 1 one ulp of p moves it by 6e-8 / (1 - p), so the distance grows with
# the band.  Beyond |x| <= 8 the comparison stops meaning anything (2.9 at randn * 8); the saturated band is held to the
# envelope of cost_envelope() instead.
COST_MEASURED = {"4": 8.2e-6, "8": 3.4e-4}
# The saturated band: the kernel's value lies between the smallest and the largest value the oracle's float32 formula takes
# with p moved by up to +-SAT_ULPS ulps, widened by the |x| <= 8 limit.  1 / (1 + expf(-x)) rounds 1 + e to a spacing of
# 1.2e-7, two ulps of a p just below 1, before the division rounds once more.  Observed on the MI355X: two ulps were not
# needed, every entry of the four cases already lies within the widened k = 0 envelope (the oracle's own float32 value)
# while being up to 2.85 away from float64.
SAT_ULPS = 2

# max |float32 restatement - float64| / max(1, |float64|) per tracker kernel and mode, measured on the CPU like COST_MEASURED
TRACKER_MEASURED = {"cost": 1.0e-7, "extrapolate_none": 7.1e-8, "extrapolate_linear": 7.1e-8,
                    "extrapolate_percentual": 1.3e-7, "extrapolate_average": 7.1e-8}


def cost_limit(band):
    """(atol, rtol) of a moderate band ("4" or "8")."""
    return max(COST_TOL[0], MEASURED_FACTOR * COST_MEASURED[band]), COST_TOL[1]


def tracker_limit(op):
    """On |got - ref| / max(1, |ref|).  One figure per kernel and mode, the largest over its cases: the 1 x 1 case alone
    can measure 0."""
    return MEASURED_FACTOR * TRACKER_MEASURED[op]


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _random_boxes(g, shape, kind):
    """cxcywh in (0, 1): predictions and targets as test_matcher_and_losses draws them."""
    if kind == "pred":
        return torch.rand(*shape, 4, generator=g) * 0.5 + 0.1
    cxcy = torch.rand(*shape, 2, generator=g) * 0.6 + 0.2
    return torch.cat([cxcy, torch.rand(*shape, 2, generator=g) * 0.3 + 0.02], -1)


# ------------------------------------------------------------------------------------------------ box geometry
# (pred, target) in cxcywh, every coordinate a multiple of 1/64 (1/1024 for the tiny target): exact in float32, and so are
# the corners, so float32 and float64 take the same min / max / clamp branches.
_D = 1 / 64
GEOMETRY = {
    "disjoint_x":        ([16 * _D, 32 * _D, 16 * _D, 32 * _D], [48 * _D, 32 * _D, 16 * _D, 16 * _D]),
    "disjoint_y":        ([32 * _D, 16 * _D, 32 * _D, 16 * _D], [32 * _D, 48 * _D, 16 * _D, 16 * _D]),
    "disjoint_xy":       ([16 * _D, 16 * _D, 16 * _D, 16 * _D], [48 * _D, 50 * _D, 16 * _D, 8 * _D]),
    "pred_inside":       ([32 * _D, 32 * _D, 16 * _D, 16 * _D], [34 * _D, 30 * _D, 32 * _D, 48 * _D]),
    "target_inside":     ([34 * _D, 30 * _D, 32 * _D, 48 * _D], [32 * _D, 32 * _D, 16 * _D, 16 * _D]),
    "identical":         ([32 * _D, 32 * _D, 16 * _D, 32 * _D], [32 * _D, 32 * _D, 16 * _D, 32 * _D]),   # loss 0, all ties
    "shared_x0":         ([24 * _D, 32 * _D, 16 * _D, 32 * _D], [32 * _D, 32 * _D, 32 * _D, 16 * _D]),   # x0 = 1/4 in both
    "touching_x":        ([16 * _D, 32 * _D, 32 * _D, 32 * _D], [48 * _D, 32 * _D, 32 * _D, 16 * _D]),   # raw iw == 0, ih > 0
    "touching_y":        ([32 * _D, 16 * _D, 32 * _D, 32 * _D], [32 * _D, 48 * _D, 16 * _D, 32 * _D]),   # raw ih == 0, iw > 0
    "tiny_target":       ([32 * _D, 32 * _D, 16 * _D, 16 * _D], [33 * _D, 32 * _D, 1 / 1024, 1 / 1024]),
    "zero_width_target": ([32 * _D, 32 * _D, 32 * _D, 32 * _D], [33 * _D, 32 * _D, 0.0, 16 * _D]),        # union = pred area
}
# The pairs appended to the larger cases.  At a touching pair the kernel follows autograd's subgradient only since
# giou_loss_grad tests `raw >= 0`; those two are pinned by their own cases, nothing else depends on them.
APPENDED = tuple(k for k in GEOMETRY if not k.startswith("touching"))

# ------------------------------------------------------------------------------------------------ set losses
# counts:   targets per sample (the same in every level); M = every query matched
# num_boxes: None -- max(sum(counts), 1), what the criterion passes on one rank; a number -- a multi-rank mean
# band:     "moderate" randn * 2 - 2 | "saturated" randn * 8 with rows holding +-30, +-88, +-104 (expf(104) overflows)
# geometry: None | the sample that gets the APPENDED pairs as its last targets, matched to its last queries
#           | the name of ONE pair (M = 1 cases; the same pair in both levels)
LossCase = namedtuple("LossCase", "name L B M C counts num_boxes alpha band geometry")
LOSS_CASES = {}


def _loss(name, L, B, M, C, counts, num_boxes=None, alpha=0.25, band="moderate", geometry=None):
    assert name not in LOSS_CASES and len(counts) == B and max(counts) <= M
    LOSS_CASES[name] = LossCase(name, L, B, M, C, tuple(counts), num_boxes, alpha, band, geometry)


_loss("m1", 1, 1, 1, 1, [1])                                                     # one thread does everything
_loss("m1_empty", 1, 1, 1, 3, [0], alpha=0.6)
_loss("m255", 3, 3, 255, 3, [0, 1, 255], alpha=0.6, band="saturated")            # one trip, one idle thread
_loss("m256", 1, 1, 256, 8, [256], geometry=0)                                   # exactly one trip
_loss("m257", 3, 3, 257, 10, [40, 0, 257], num_boxes=36.5, geometry=0)           # the second trip has one row
_loss("m300", 1, 3, 300, 91, [17, 1, 300], band="saturated", geometry=2)         # the default query count, COCO's classes
_loss("m513", 3, 3, 513, 3, [0, 513, 30], alpha=0.6)                             # three trips
_loss("all_empty", 3, 3, 300, 8, [0, 0, 0], band="saturated")                    # nm = 0: class_error 100, num_boxes 1
for _k in GEOMETRY:
    _loss("pair_" + _k, 2, 1, 1, 1, [1], geometry=_k)              # two levels: the L1 weight is 0 only in the first

LossData = namedtuple("LossData", "case logits boxes match tl tb toff num_boxes g")

SATURATED_VALUES = (30.0, -30.0, 88.0, -88.0, 104.0, -104.0)
HALF_UP = float(np.nextafter(np.float32(0.5), np.float32(1)))


def build_loss_case(name):
    """-> LossData, all float32 / int on the CPU.  match[l, b, m] is the GLOBAL target index or -1: per level and sample the
    scipy assignment of the float64 cost (the matcher stays out of the loss tests), then the hand-built pairs."""
    c = LOSS_CASES[name]
    g = _gen("loss " + name)
    L, B, M, C = c.L, c.B, c.M, c.C
    scale, shift = (2.0, -2.0) if c.band == "moderate" else (8.0, 0.0)
    logits = torch.randn(L, B, M, C, generator=g) * scale + shift
    boxes = _random_boxes(g, (L, B, M), "pred")
    if M >= 8:
        # cardinality counts rows whose largest LOGIT exceeds 0.5: row 0 sits on the threshold, row 1 one ulp above it
        for row, top in ((0, 0.5), (1, HALF_UP)):
            logits[:, :, row] = logits[:, :, row].clamp(max=0.25)
            logits[:, :, row, 0] = top
        if c.band == "saturated":
            for k, v in enumerate(SATURATED_VALUES):
                logits[:, :, 2 + k, k % C] = v
                if C > 1:
                    logits[:, :, 2 + k, (k + 1) % C] = -v
    pairs = []
    if isinstance(c.geometry, str):
        pairs = [c.geometry]
    elif c.geometry is not None:
        pairs = list(APPENDED)
        assert c.counts[c.geometry] >= len(pairs)
    tl, tb, toff = [], [], [0]
    for b, n in enumerate(c.counts):
        has = bool(pairs) and (isinstance(c.geometry, str) or b == c.geometry)
        nr = n - (len(pairs) if has else 0)
        lab = torch.randint(0, C, (nr,), generator=g)
        if nr:
            lab[0] = C - 1                                                       # the last class is a label
        bx = _random_boxes(g, (nr,), "target")
        if has:
            lab = torch.cat([lab, torch.arange(len(pairs)) % C])
            bx = torch.cat([bx, torch.tensor([GEOMETRY[k][1] for k in pairs], dtype=torch.float32)])
            boxes[:, b, M - len(pairs):] = torch.tensor([GEOMETRY[k][0] for k in pairs], dtype=torch.float32)
        tl.append(lab); tb.append(bx); toff.append(toff[-1] + n)
    tl, tb = torch.cat(tl), torch.cat(tb)
    match = torch.full((L, B, M), -1, dtype=torch.int32)
    if toff[-1]:
        for lv in range(L):
            cost = tp.matcher_cost_matrix(logits[lv].double(), boxes[lv].double(), tl, tb.double(), 2.0, 5.0, 2.0,
                                          alpha=c.alpha)
            for b, n in enumerate(c.counts):
                has = bool(pairs) and (isinstance(c.geometry, str) or b == c.geometry)
                ng = len(pairs) if has else 0
                if n - ng:
                    i, j = linear_sum_assignment(cost[b, :M - ng, toff[b]:toff[b] + n - ng].numpy())
                    match[lv, b, torch.as_tensor(i)] = torch.as_tensor(j + toff[b], dtype=torch.int32)
                for k in range(ng):
                    match[lv, b, M - ng + k] = toff[b] + n - ng + k
    assert [int((match[0, b] >= 0).sum()) for b in range(B)] == list(c.counts)
    assert_no_tied_top_logits(logits, match)
    num_boxes = float(c.num_boxes) if c.num_boxes is not None else max(float(toff[-1]), 1.0)
    # backward weights: distinct per level and loss, one exactly 0, one negative
    w = torch.rand(L, 3, generator=g) + 0.5
    w[0, 1] = 0.0
    w[L - 1, 2] = -0.75
    return LossData(c, logits, boxes, match, tl, tb, torch.tensor(toff, dtype=torch.int32), num_boxes, w)


def assert_no_tied_top_logits(logits, match):
    """class_error comes from topk, whose order among tied logits is unspecified: matched rows have one largest logit."""
    if logits.shape[-1] < 2:
        return
    top = logits[match >= 0].topk(2, -1)[0]
    assert bool((top[:, 0] > top[:, 1]).all()), "a matched row has tied top logits"


def loss_reference(d, dtype=torch.float64):
    """-> (out [L, 5], dlogits, dboxes) of oracle/criterion.py at `dtype`; the gradients are those of
    sum_l g[l, 0] * loss_ce + g[l, 1] * loss_bbox + g[l, 2] * loss_giou."""
    c = d.case
    cfg = O.Config(focal_alpha=c.alpha)
    logits = d.logits.to(dtype).requires_grad_(True)
    boxes = d.boxes.to(dtype).requires_grad_(True)
    toff = d.toff.tolist()
    targets = [{"labels": d.tl[toff[b]:toff[b + 1]], "boxes": d.tb[toff[b]:toff[b + 1]].to(dtype)} for b in range(c.B)]
    out, total = [], 0.0
    for lv in range(c.L):
        indices = []
        for b in range(c.B):
            src = torch.nonzero(d.match[lv, b] >= 0).flatten()
            indices.append((src, d.match[lv, b, src].long() - toff[b]))
        ld = ocrit.loss_labels(cfg, logits[lv], targets, indices, d.num_boxes)
        ld.update(ocrit.loss_boxes(boxes[lv], targets, indices, d.num_boxes))
        ld.update(ocrit.loss_cardinality(logits[lv], targets))
        out.append(torch.stack([ld[k].detach().to(dtype) for k in
                                ("loss_ce", "loss_bbox", "loss_giou", "cardinality_error", "class_error")]))
        total = total + d.g[lv, 0].to(dtype) * ld["loss_ce"] + d.g[lv, 1].to(dtype) * ld["loss_bbox"] \
            + d.g[lv, 2].to(dtype) * ld["loss_giou"]
    grads = torch.autograd.grad(total, [logits, boxes], allow_unused=True)
    dl, db = (torch.zeros_like(x) if gr is None else gr for x, gr in zip((logits, boxes), grads))
    return torch.stack(out), dl, db


def within(got, ref, tol):
    """(ok, worst |got - ref| - (atol + rtol |ref|)) in float64."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    over = (got - ref).abs() - (tol[0] + tol[1] * ref.abs())
    worst = float(over.max()) if over.numel() else -tol[0]
    return bool(torch.isfinite(got).all()) and worst <= 0.0, worst


def check_loss(got, ref, tag=""):
    """got / ref: (out [L, 5], dlogits, dboxes).  Every figure is finite and within LOSS_TOL of the reference."""
    out, dl, db = got
    rout, rdl, rdb = ref
    for what, a, b, tol in (("losses", out[:, :3], rout[:, :3], LOSS_TOL["loss"]),
                            ("class_error", out[:, 4], rout[:, 4], LOSS_TOL["class_error"]),
                            ("dlogits", dl, rdl, LOSS_TOL["dlogits"]), ("dboxes", db, rdb, LOSS_TOL["dboxes"])):
        ok, worst = within(a, b, tol)
        assert ok, f"{tag}{what}: off the limit by {worst:.3e}\n got {a.flatten()[:8]}\n ref {b.flatten()[:8]}"
    assert torch.equal(out[:, 3].double().cpu(), rout[:, 3].double()), f"{tag}cardinality_error {out[:, 3]} vs {rout[:, 3]}"


# ------------------------------------------------------------------------------------------------ match cost
# rows = L * B * M: four rows share a workgroup.  counts: one wave strides over a sample's targets 64 at a time.
CostCase = namedtuple("CostCase", "name L B M C counts ld weights alpha gamma")
COST_CASES = {}
COST_BANDS = ("4", "8", "saturated")


def _cost(name, L, B, M, C, counts, ld, weights=(2.0, 5.0, 2.0), alpha=0.25, gamma=2.0):
    assert len(counts) == B and ld > max(counts)
    COST_CASES[name] = CostCase(name, L, B, M, C, tuple(counts), ld, weights, alpha, gamma)


_cost("rows1", 1, 1, 1, 1, [1], 4)                                                           # rows % 4 == 1
_cost("rows6", 1, 2, 3, 10, [0, 65], 72, weights=(1.0, 3.0, 0.5), alpha=0.6, gamma=1.5)      # rows % 4 == 2
_cost("rows15", 1, 3, 5, 91, [64, 1, 130], 136, weights=(2.5, 4.0, 1.5), alpha=0.6)          # rows % 4 == 3
_cost("rows1800", 3, 2, 300, 10, [130, 0], 131, gamma=1.5)                                   # the default query count

CostData = namedtuple("CostData", "case band logits boxes tl tb toff")


def build_cost_case(name, band):
    c = COST_CASES[name]
    g = _gen(f"cost {name} {band}")
    shape = (c.L, c.B, c.M, c.C)
    if band == "saturated":
        logits = (torch.randn(*shape, generator=g) * 8).clamp(-30.0, 30.0)
        logits[:, :, ::3] = (torch.rand(*shape, generator=g)[:, :, ::3] * 2 - 1) * 30
        logits[:, :, 0, 0] = 30.0
        logits[:, :, 0, c.C - 1] = -30.0 if c.C > 1 else 30.0
    else:
        logits = (torch.rand(*shape, generator=g) * 2 - 1) * float(band)
    boxes = _random_boxes(g, shape[:3], "pred")
    tl, toff = [], [0]
    for n in c.counts:
        lab = torch.randint(0, c.C, (n,), generator=g)
        if n:
            lab[-1] = c.C - 1
        tl.append(lab); toff.append(toff[-1] + n)
    tb = _random_boxes(g, (toff[-1],), "target")
    return CostData(c, band, logits, boxes, torch.cat(tl), tb, torch.tensor(toff, dtype=torch.int32))


def _pad_cost(d, full):
    """[L, B, M, sum n] (every sample against every target) -> the kernel's layout [L, B, M, ld], zeros past a sample's count."""
    c = d.case
    out = torch.zeros(c.L, c.B, c.M, c.ld, dtype=full.dtype)
    toff = d.toff.tolist()
    for b, n in enumerate(c.counts):
        out[:, b, :, :n] = full[:, b, :, toff[b]:toff[b + 1]]
    return out


def cost_valid(d):
    """bool [ld] per sample -> [1, B, 1, ld]: the columns the kernel writes."""
    return (torch.arange(d.case.ld)[None, :] < torch.tensor(d.case.counts)[:, None])[None, :, None, :]


def cost_reference(d, dtype=torch.float64):
    c = d.case
    wc, wb, wg = c.weights
    full = torch.stack([tp.matcher_cost_matrix(d.logits[lv].to(dtype), d.boxes[lv].to(dtype), d.tl, d.tb.to(dtype),
                                               wc, wb, wg, alpha=c.alpha, gamma=c.gamma) for lv in range(c.L)])
    return _pad_cost(d, full)


def _shift_ulps(p, k):
    toward = torch.full_like(p, 2.0 if k > 0 else -1.0)
    for _ in range(abs(k)):
        p = torch.nextafter(p, toward)
    return p.clamp(0.0, 1.0)


def cost_envelope(d, ulps=SAT_ULPS):
    """(lo, hi) [L, B, M, ld] float32: oracle/thirdparty.matcher_cost_matrix's float32 expression with the sigmoid moved by
    -ulps .. +ulps float32 steps (0 is the oracle itself)."""
    c = d.case
    wc, wb, wg = c.weights
    lo = hi = None
    for lv in range(c.L):
        p0 = d.logits[lv].flatten(0, 1).sigmoid()
        bx = d.boxes[lv].flatten(0, 1)
        rest = wb * torch.cdist(bx, d.tb, p=1)
        c_giou = -tp.generalized_box_iou(tp.box_cxcywh_to_xyxy(bx), tp.box_cxcywh_to_xyxy(d.tb))
        vals = []
        for k in range(-ulps, ulps + 1):
            p = _shift_ulps(p0, k)
            neg = (1 - c.alpha) * (p ** c.gamma) * (-(1 - p + 1e-8).log())
            pos = c.alpha * ((1 - p) ** c.gamma) * (-(p + 1e-8).log())
            vals.append((rest + wc * (pos[:, d.tl] - neg[:, d.tl]) + wg * c_giou).view(c.B, c.M, -1))
        vals = torch.stack(vals)
        lo_l, hi_l = vals.amin(0), vals.amax(0)
        lo = lo_l[None] if lo is None else torch.cat([lo, lo_l[None]])
        hi = hi_l[None] if hi is None else torch.cat([hi, hi_l[None]])
    return _pad_cost(d, lo), _pad_cost(d, hi)


def envelope_excess(got, d, ulps=SAT_ULPS):
    """How far `got` lies outside the envelope widened by the |x| <= 8 limit (<= 0: inside), over the written columns."""
    lo, hi = cost_envelope(d, ulps)
    atol, rtol = cost_limit("8")
    got = got.double().cpu()
    lo, hi = lo.double(), hi.double()
    over = torch.maximum(lo - got - (atol + rtol * lo.abs()), got - hi - (atol + rtol * hi.abs()))
    return float(over[cost_valid(d).expand_as(over)].max())


def measure_cost_band(band):
    """max |float32 oracle - float64| over the COST_CASES of a moderate band."""
    worst = 0.0
    for name in COST_CASES:
        d = build_cost_case(name, band)
        worst = max(worst, float((cost_reference(d, torch.float32).double() - cost_reference(d)).abs().max()))
    return worst


# ------------------------------------------------------------------------------------------------ tracker baseline
TRACKER_COST_CASES = {"strided": (2, 300, 900, 3), "one": (1, 1, 1, 1)}        # 540 000 elements > 2048 * 256: the grid strides
TRACKER_MODES = (None, "linear", "percentual", "average")
TRACKER_FACTORS = ("none", "per_sample")
TrackerData = namedtuple("TrackerData", "b2 l2 b1 l1 mapping factor")


def build_tracker_case(name, B, M, N, C):
    g = _gen("tracker " + name)
    b2, b1 = _random_boxes(g, (B, M), "pred"), _random_boxes(g, (B, N), "pred")       # sizes in [0.1, 0.6]: away from 0
    l2, l1 = torch.randn(B, M, C, generator=g) * 2, torch.randn(B, N, C, generator=g) * 2
    mapping = torch.randint(0, N, (B, M), generator=g).int()
    mapping[:, ::3] = -1                                                              # unmatched rows, the first included
    factor = torch.tensor([0.0, -0.5, 1.75])[:B]                                      # 0 and a negative factor
    return TrackerData(b2, l2, b1, l1, mapping, factor)


TRACKER_EXTRAPOLATE_SHAPE = (3, 70, 40, 5)


def tracker_cost_reference(d, dtype=torch.float64):
    """The two cdist terms of oracle/stdetr.tracker_future_predictor written out: Euclidean distance of the centres and the
    largest difference of the class probabilities."""
    b2, b1, s2, s1 = d.b2.to(dtype), d.b1.to(dtype), d.l2.to(dtype).sigmoid(), d.l1.to(dtype).sigmoid()
    dist = ((b2[:, :, None, 0:2] - b1[:, None, :, 0:2]) ** 2).sum(-1).sqrt()
    return 0.5 * dist + 0.5 * (s2[:, :, None] - s1[:, None]).abs().amax(-1)


def tracker_extrapolate_reference(d, mode, with_factor, dtype=torch.float64):
    """oracle/stdetr.tracker_future_predictor from the mapping on, at `dtype` -> (boxes, logits)."""
    b2, b1, l2, l1 = d.b2.to(dtype), d.b1.to(dtype), d.l2.to(dtype), d.l1.to(dtype)
    f = d.factor.to(dtype)[:, None, None] if with_factor else 1.0
    has = d.mapping != -1
    idx = d.mapping.long().clamp(min=0)
    c1 = b1.gather(1, idx[:, :, None].expand(-1, -1, 4)).clone()
    c1[~has] = b2[~has]
    if mode is None:
        dims = b2[..., 2:4]
    elif mode == "linear":
        dims = torch.clamp(b2[..., 2:4] + (b2[..., 2:4] - c1[..., 2:4]) * f, min=0)
    elif mode == "percentual":
        dims = b2[..., 2:4] * (b2[..., 2:4] / c1[..., 2:4]) ** f
    else:
        dims = (b2[..., 2:4] + c1[..., 2:4]) / 2
    pos = b2[..., 0:2] + (b2[..., 0:2] - c1[..., 0:2]) * f
    cl = l1.gather(1, idx[..., None].expand(-1, -1, l1.shape[-1])).clone()
    cl[~has] = 0.0
    return torch.cat([pos, dims], dim=2), 0.5 * (l2 + cl)


def scaled_error(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float(((got - ref).abs() / ref.abs().clamp(min=1.0)).max())


def measure_tracker(op):
    if op == "cost":
        worst = 0.0
        for name, shape in TRACKER_COST_CASES.items():
            d = build_tracker_case(name, *shape)
            worst = max(worst, scaled_error(tracker_cost_reference(d, torch.float32), tracker_cost_reference(d)))
        return worst
    mode = {"none": None}.get(op[len("extrapolate_"):], op[len("extrapolate_"):])
    d = build_tracker_case("extrapolate", *TRACKER_EXTRAPOLATE_SHAPE)
    worst = 0.0
    for with_factor in (False, True):
        a, b = tracker_extrapolate_reference(d, mode, with_factor, torch.float32), tracker_extrapolate_reference(d, mode, with_factor)
        worst = max(worst, scaled_error(a[0], b[0]), scaled_error(a[1], b[1]))
    return worst


# ------------------------------------------------------------------------------------------------ post-processing
POST_PROC_CASES = ((1, 1), (257, 10), (600, 1), (600, 10))                       # (R, C): one thread, a second block, three
