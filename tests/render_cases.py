"""Cases for the box renderer (include/fod_ext.h: fod_render_boxes) and an independent numpy restatement of its map,
shared by tests/test_render_cpu.py, tests/test_render_gpu.py and tests/golden/make_render_golden.py.  The restatement
paints in box order with array slicing, float32 arithmetic and explicit truncation; it shares no helper with the
package.

A case is a dict: name, video (numpy f32 or uint8 [B, L, 3, H, W]), boxes f32 [B, N, 4], labels i32 [B, N],
frame_idx (list of B ints, or None), thickness, gap (elements between the clips of consecutive samples in memory)."""
import numpy as np

MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)
LEVELS = (0, 63, 127, 191, 255)                      # trunc(lv * 255) of lv = 0, .25, .5, .75, 1
PALETTE = np.array([[LEVELS[c], LEVELS[b], LEVELS[a]] for a in range(5) for b in range(5) for c in range(5)],
                   dtype=np.uint8)                  # [125, 3]
P = len(PALETTE)
SIZES = ((17, 23), (24, 40))                         # W % 4 != 0 (and rows that are not 16-byte aligned); all aligned
WIDE = (18, 262)                                     # two tile columns, two tile rows, W % 4 == 2
INF, NAN = float("inf"), float("nan")


# ---- the restatement -------------------------------------------------------------------------------------------------
def background(frame):
    """[3, H, W] f32 normalised or uint8 -> uint8 [H, W, 3]."""
    if frame.dtype == np.uint8:
        return np.ascontiguousarray(frame.transpose(1, 2, 0))
    assert frame.dtype == np.float32
    with np.errstate(all="ignore"):
        v = frame * STD[:, None, None]               # each step a float32 array operation: rounded to f32
        v = v + MEAN[:, None, None]
        w = v * np.float32(255)
        assert w.dtype == np.float32
        w = np.where(np.isfinite(w), w, np.float32(0))
        w = np.trunc(w)
        w = np.minimum(np.maximum(w, np.float32(0)), np.float32(255))
    return np.ascontiguousarray(w.astype(np.uint8).transpose(1, 2, 0))


def edge(v, t, extent):
    v = np.float32(v)
    v = np.maximum(v, np.float32(t))
    v = np.minimum(v, np.float32(extent - t))
    return int(np.trunc(v))


def paint(img, boxes, labels, t, palette=PALETTE):
    """img uint8 [H, W, 3], in place: every drawn box in index order, later ones on top."""
    H, W, _ = img.shape
    for box, label in zip(boxes, labels):
        if not 0 <= int(label) < len(palette) or np.isnan(box).any():
            continue
        lf, tp, rt, bt = edge(box[0], t, W), edge(box[1], t, H), edge(box[2], t, W), edge(box[3], t, H)
        colour = palette[int(label)]
        img[tp - t:bt, lf - t:lf] = colour           # left
        img[bt:bt + t, lf - t:rt] = colour           # bottom
        img[tp:bt + t, rt:rt + t] = colour           # right
        img[tp - t:tp, lf:rt + t] = colour           # top
    return img


def frame_of(case, b):
    L = case["video"].shape[1]
    f = 0 if case["frame_idx"] is None else case["frame_idx"][b]
    if f < 0:
        f += L
    return min(max(f, 0), L - 1)


def expected(case):
    """uint8 [B, H, W, 3]"""
    out = []
    for b in range(case["video"].shape[0]):
        img = background(case["video"][b, frame_of(case, b)])
        out.append(paint(img, case["boxes"][b], case["labels"][b], case["thickness"]))
    return np.stack(out)


# ---- the cases ---------------------------------------------------------------------------------------------------------
def _video(B, L, H, W, seed):
    return np.random.default_rng(seed).standard_normal((B, L, 3, H, W)).astype(np.float32)


def _case(name, H, W, t, boxes, labels, B=1, L=1, frame_idx=None, gap=0, video=None, seed=0):
    boxes = np.asarray(boxes, dtype=np.float32).reshape(B, -1, 4)
    labels = np.asarray(labels, dtype=np.int32).reshape(B, -1)
    assert boxes.shape[1] == labels.shape[1]
    video = _video(B, L, H, W, seed) if video is None else video
    return dict(name=f"{name} {H}x{W} t{t}", video=video, boxes=boxes, labels=labels, frame_idx=frame_idx, thickness=t,
                gap=gap)


def _random_boxes(n, H, W, seed):
    g = np.random.default_rng(seed)
    xy = g.uniform(-4, 1, (n, 2)) + g.uniform(0, 1, (n, 2)) * np.array([W, H])
    wh = g.uniform(0, 1, (n, 2)) * np.array([W, H]) * 0.6
    return np.concatenate([xy, xy + wh], axis=1).astype(np.float32), g.integers(0, P, n).astype(np.int32)


def geometry_cases():
    out = []
    for H, W in SIZES:
        for t in (1, 3):
            c = lambda name, boxes, labels, **kw: out.append(_case(name, H, W, t, boxes, labels, **kw))
            c("no boxes", np.zeros((0, 4)), np.zeros(0))
            c("interior", [[6.2, 5.1, W - 7.5, H - 6.3]], [31])
            c("borders and outside", [[-5, 4, 9, 11], [W - 6, 3, W + 9, 12], [5, -7, 14, 6], [4, H - 5, 15, H + 20],
                                      [W + 30, H + 30, W + 60, H + 60], [-80, -90, -10, -20]], [1, 5, 25, 30, 62, 124])
            c("reversed", [[W - 6, 4, 7, H - 5], [5, H - 4, W - 8, 6], [W - 9, H - 6, 8, 5]], [7, 43, 99])
            c("zero area", [[10, 8, 10, 8], [12.5, 3, 12.5, 13], [3, 9.9, 18, 9.9]], [100, 101, 102])
            c("overlapping: last wins", [[4, 4, 16, 12], [8, 6, 20, 14], [4, 4, 16, 12], [6, 4, 18, 12]], [3, 60, 90, 17])
            boxes, labels = _random_boxes(70, H, W, 70 + t)
            c("70 boxes", boxes, labels)
            boxes, labels = _random_boxes(1024, H, W, 1024 + t)
            c("1024 boxes", boxes, labels)
            below, above = np.nextafter(np.float32(9), np.float32(0)), np.nextafter(np.float32(9), np.float32(99))
            c("fractions around an integer", [[below, above, 15.999999, 12.000001], [above, below, 16.000002, 11.999999]],
              [44, 88])
            c("infinite", [[-INF, 5, 12, INF], [6, -INF, INF, 10], [-INF, -INF, INF, INF], [INF, INF, -INF, -INF]],
              [9, 19, 29, 39])
            c("NaN coordinate: skipped", [[5, 5, 12, 12], [NAN, 4, 15, 13], [6, 4, NAN, 13], [6, NAN, 15, 13],
                                          [6, 4, 15, NAN], [7, 7, 14, 10]], [50, 51, 52, 53, 54, 55])
            c("labels -1 and P: skipped", [[5, 5, 12, 12], [4, 4, 15, 13], [6, 3, 16, 11], [7, 7, 14, 10]],
              [-1, P, 77, -2147483648])
            b0, l0 = _random_boxes(5, H, W, 5 + t)
            b1, l1 = _random_boxes(5, H, W, 6 + t)
            c("two samples, frames (-1, 1)", np.stack([b0, b1]), np.stack([l0, l1]), B=2, L=3, frame_idx=[-1, 1], seed=2)
            c("frame index out of range: clamped", np.stack([b0, b1]), np.stack([l0, l1]), B=2, L=3, frame_idx=[7, -9],
              seed=3)
            c("batch stride gap", np.stack([b1, b0]), np.stack([l1, l0]), B=2, L=2, frame_idx=[1, 0], gap=5, seed=4)
    H, W = WIDE
    boxes, labels = _random_boxes(40, H, W, 40)
    out.append(_case("wide: boxes across the tile edge", H, W, 3,
                     np.concatenate([[[250, 2, 262, 16], [3, 14, 258, 17], [255.5, 1, 256.5, 17], [259, 15, 240, 3]], boxes]),
                     np.concatenate([[11, 22, 33, 66], labels])))
    return out


def pixel_cases():
    """f32 values that de-normalise below 0, above 1 and to exact multiples of 1/255; a NaN and both infinities."""
    H, W, t = SIZES[0]  + (3,)
    video = _video(1, 1, H, W, 9) * np.float32(4)                      # many pixels leave 0..1 on both sides
    k = np.arange(H * W, dtype=np.float32).reshape(H, W) % 256
    for c in range(3):                                                 # plane c, rows 0..7: x with x * std + mean ~ k / 255
        video[0, 0, c, :8] = ((k / np.float32(255) - MEAN[c]) / STD[c])[:8]
    video[0, 0, 0, 9, 3], video[0, 0, 1, 9, 4], video[0, 0, 2, 9, 5], video[0, 0, 1, 10, 20] = NAN, INF, -INF, 3.0e38
    out = [_case("pixels", H, W, t, [[6, 11, 17, 15]], [13], video=video)]
    u8 = np.random.default_rng(11).integers(0, 256, (2, 2, 3, 24, 40), dtype=np.uint8)
    boxes, labels = _random_boxes(6, 24, 40, 12)
    out.append(_case("uint8 source", 24, 40, 3, np.stack([boxes, boxes[::-1]]), np.stack([labels, labels[::-1]]), B=2, L=2,
                     frame_idx=[1, -2], video=u8))
    u8 = np.random.default_rng(13).integers(0, 256, (1, 1, 3, 17, 23), dtype=np.uint8)
    out.append(_case("uint8 source, unaligned rows", 17, 23, 1, boxes[:3], labels[:3], video=u8))
    return out


def all_cases():
    return geometry_cases() + pixel_cases()
