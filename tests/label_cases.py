"""Cases for the captions (include/fod_ext.h: fod_render_labels) and an independent numpy restatement of its map, shared
by tests/test_labels_cpu.py and tests/test_labels_gpu.py.  The restatement loops over the labels in index order, over
the characters of a text and over the pixels of a glyph, and paints with array slicing (a slice that leaves the picture
is clipped by numpy); it shares no helper with the package.  The 5x7 font is data the package owns, so the callers hand
it in: `all_cases(font_5x7)`.

A case is a dict: name, picture (uint8 [B, H, W, 3], random bytes: what the captions are painted on), boxes f32
[B, N, 4], labels i32 [B, N], idents i32 [B, N] or None, scores f32 [B, N] or None, names uint8 [n_names, stride] or
None, palette uint8 [P, 3], font uint8 [G, FH], font_first, font_width, scale, thickness."""
import numpy as np

MAX_CHARS = 32
LEVELS = (0, 63, 127, 191, 255)
PALETTE = np.array([[LEVELS[c], LEVELS[b], LEVELS[a]] for a in range(5) for b in range(5) for c in range(5)],
                   dtype=np.uint8)                  # [125, 3]: entry 0 is black, entry 124 white
P = len(PALETTE)
SIZES = ((18, 262), (40, 300), (24, 40))             # two tile columns and W % 4 != 0, twice; one aligned picture
INF, NAN = float("inf"), float("nan")
LONG_NAME = "a_name_of_exactly_32_bytes_here!"       # fills its row: no terminating 0
NAME_LIST = ["car", "ConstructionVehicle", "pedestrian", "", LONG_NAME, "Bus~{|}", "x", "Trailer_07"]
assert len(LONG_NAME) == MAX_CHARS


def name_table(names):
    stride = max(len(n) for n in names)
    table = np.zeros((len(names), stride), dtype=np.uint8)
    for i, n in enumerate(names):
        table[i, :len(n)] = np.frombuffer(n.encode("ascii"), dtype=np.uint8)
    return table


NAMES = name_table(NAME_LIST)                        # [8, 32]


# ---- the restatement -------------------------------------------------------------------------------------------------
def text_of(ident, label, score, names):
    """The bytes of one caption; ident / score / names None where the operand is absent."""
    parts = []
    if ident is not None and int(ident) >= 0:
        parts.append(b"%d" % int(ident))
    if names is not None and 0 <= int(label) < len(names):
        row = names[int(label)].tobytes()
        end = row.find(b"\0")
        parts.append(row if end < 0 else row[:end])
    if score is not None and not np.isnan(score):
        with np.errstate(all="ignore"):
            p = np.float32(score) * np.float32(100)
        assert p.dtype == np.float32
        pct = int(np.trunc(np.minimum(np.maximum(p, np.float32(0)), np.float32(99))))
        parts.append(b"%d%d" % (pct // 10, pct % 10))
    return b" ".join(parts)[:MAX_CHARS]


def edge(v, t, extent):
    v = np.float32(v)
    v = np.maximum(v, np.float32(t))
    v = np.minimum(v, np.float32(extent - t))
    return int(np.trunc(v))


def paint(img, boxes, labels, idents, scores, names, palette, font, first, FW, s, t):
    """img uint8 [H, W, 3], in place: every drawn label in index order, later plates on top."""
    H, W, _ = img.shape
    FH = font.shape[1]
    for n in range(len(labels)):
        label = int(labels[n])
        if not 0 <= label < len(palette) or np.isnan(boxes[n]).any():
            continue
        text = text_of(None if idents is None else idents[n], label, None if scores is None else scores[n], names)
        if not text:
            continue
        Wp, Hp = (len(text) * (FW + 1) + 1) * s, (FH + 2) * s
        x0, y0 = edge(boxes[n][0], t, W) - t, edge(boxes[n][1], t, H) - t - Hp
        if y0 < 0:
            y0 = edge(boxes[n][1], t, H)
        x0, y0 = max(min(x0, W - Wp), 0), max(min(y0, H - Hp), 0)
        r, g, b = (int(c) for c in palette[label])
        ink = (0, 0, 0) if 299 * r + 587 * g + 114 * b >= 128000 else (255, 255, 255)
        img[y0:y0 + Hp, x0:x0 + Wp] = palette[label]
        for i, code in enumerate(text):
            if not first <= code < first + len(font):
                continue                             # no glyph: a blank cell
            for v in range(FH):
                for col in range(FW):
                    if int(font[code - first, v]) >> (7 - col) & 1:
                        ya, xa = y0 + (1 + v) * s, x0 + (1 + i * (FW + 1) + col) * s
                        img[ya:ya + s, xa:xa + s] = ink
    return img


_EXPECTED = {}


def expected(case):
    """uint8 [B, H, W, 3]; computed once per case and handed out read-only."""
    hit = _EXPECTED.get(case["name"])
    if hit is None:
        out = case["picture"].copy()
        pick = lambda key, b: None if case[key] is None else case[key][b]
        for b in range(out.shape[0]):
            paint(out[b], case["boxes"][b], case["labels"][b], pick("idents", b), pick("scores", b), case["names"],
                  case["palette"], case["font"], case["font_first"], case["font_width"], case["scale"], case["thickness"])
        out.setflags(write=False)
        hit = _EXPECTED[case["name"]] = out
    return hit


def clip_of(case):
    """The case's pictures as a raw uint8 clip [B, 1, 3, H, W]: what `render` takes."""
    return np.ascontiguousarray(case["picture"].transpose(0, 3, 1, 2)[:, None])


_OVER_OUTLINES = {}


def expected_over_outlines(case):
    """What `render(..., captions=...)` gives for a raw uint8 clip whose frame is the case's picture: the outlines of
    tests/render_cases.py's restatement first, all captions above them."""
    import render_cases as RC
    hit = _OVER_OUTLINES.get(case["name"])
    if hit is None:
        out = case["picture"].copy()
        pick = lambda key, b: None if case[key] is None else case[key][b]
        for b in range(out.shape[0]):
            RC.paint(out[b], case["boxes"][b], case["labels"][b], case["thickness"], case["palette"])
            paint(out[b], case["boxes"][b], case["labels"][b], pick("idents", b), pick("scores", b), case["names"],
                  case["palette"], case["font"], case["font_first"], case["font_width"], case["scale"], case["thickness"])
        out.setflags(write=False)
        hit = _OVER_OUTLINES[case["name"]] = out
    return hit


# ---- the cases ---------------------------------------------------------------------------------------------------------
def fonts(font_5x7):
    """name -> (font, font_first, font_width)"""
    g = np.random.default_rng(816)
    return {"5x7": (np.ascontiguousarray(font_5x7, dtype=np.uint8), 32, 5),
            "8x16 random": (g.integers(0, 256, (95, 16), dtype=np.uint8), 32, 8),
            "1x1 random": (g.integers(0, 2, (95, 1), dtype=np.uint8) * np.uint8(128), 32, 1),
            "digits only": (np.ascontiguousarray(font_5x7[16:26], dtype=np.uint8), 48, 5)}


def _case(name, H, W, font, boxes, labels, idents=None, scores=None, names=None, scale=1, t=3, B=1, palette=PALETTE,
          seed=0):
    glyphs, first, FW = font
    boxes = np.asarray(boxes, dtype=np.float32)
    N = boxes.size // (4 * B)
    boxes = boxes.reshape(B, N, 4)
    labels = np.asarray(labels, dtype=np.int32).reshape(B, N)
    idents = None if idents is None else np.asarray(idents, dtype=np.int32).reshape(B, N)
    scores = None if scores is None else np.asarray(scores, dtype=np.float32).reshape(B, N)
    picture = np.random.default_rng(1000 + seed).integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    return dict(name=f"{name} {H}x{W} s{scale} t{t}", picture=picture, boxes=boxes, labels=labels, idents=idents,
                scores=scores, names=names, palette=palette, font=glyphs, font_first=first, font_width=FW, scale=scale,
                thickness=t)


SPECIAL_SCORES = (0.0, 0.07, 0.995, 1.0, 7.0, -1.0, INF, -INF, NAN, 0.5)
SPECIAL_IDENTS = (0, 9, 10, 999, 1023, -1, 2147483647, -2147483648, 42, 7)


def _mixed(n, H, W, seed):
    """n boxes over the picture and beyond its borders, labels inside and outside the palette and the name table,
    idents and scores with the special values among them."""
    g = np.random.default_rng(seed)
    xy = g.uniform(-6, 2, (n, 2)) + g.uniform(0, 1, (n, 2)) * np.array([W, H])
    boxes = np.concatenate([xy, xy + g.uniform(0, 1, (n, 2)) * np.array([W, H]) * 0.5], axis=1).astype(np.float32)
    labels = g.integers(0, P, n).astype(np.int32)
    labels[::3] = g.integers(0, len(NAME_LIST), len(labels[::3]))        # a third of them carry a name
    idents = g.integers(0, 1024, n).astype(np.int32)
    scores = g.uniform(0, 1, n).astype(np.float32)
    k = min(n, len(SPECIAL_SCORES))
    scores[:k], idents[:k] = SPECIAL_SCORES[:k], SPECIAL_IDENTS[:k]
    return boxes, labels, idents, scores


def all_cases(font_5x7):
    F = fonts(font_5x7)
    out = []
    c = lambda *a, **kw: out.append(_case(*a, **kw))
    # every size, scale and thickness with all three parts, the default font
    for H, W in SIZES:
        for scale in (1, 2, 3, 8):
            for t in (1, 3):
                boxes, labels, idents, scores = _mixed(12, H, W, seed=H + scale + t)
                c("mixed", H, W, F["5x7"], boxes, labels, idents, scores, NAMES, scale=scale, t=t, seed=scale * 10 + t)
    # the other fonts
    for key in ("8x16 random", "1x1 random", "digits only"):
        for (H, W), scale in (((40, 300), 1), ((18, 262), 2), ((24, 40), 3)):
            boxes, labels, idents, scores = _mixed(10, H, W, seed=len(key) + scale)
            c(f"font {key}", H, W, F[key], boxes, labels, idents, scores, NAMES, scale=scale, seed=50 + scale)
    # geometry
    c("straddles a tile corner", 40, 300, F["5x7"], [[250, 26, 280, 38]], [0], [12], [0.07], NAMES)      # rows 14..22
    c("straddles a tile corner", 18, 262, F["5x7"], [[245, 9, 260, 15]], [2], [5], [0.5], NAMES, scale=2, t=1)
    for H, W in SIZES:
        c("top border: the caption moves inside", H, W, F["5x7"], [[8, 2, W - 9, H - 4], [3, 0, 20, 9]], [5, 124], [3, 4],
          [0.9, 0.1], NAMES)
        c("right border: the plate shifts left", H, W, F["5x7"], [[W - 5, H - 6, W + 4, H - 1], [W - 2, 12, W, 16]],
          [1, 0], [1023, 7], [0.99, 0.33], NAMES)
        c("bottom-left corner and outside", H, W, F["5x7"], [[-9, H - 3, 4, H + 7], [W + 40, H + 40, W + 50, H + 60],
                                                             [-70, -80, -10, -20]], [6, 7, 2], [1, 2, 3], [0.2, 0.4, 0.6],
          NAMES, t=1)
    c("plate wider and taller than the picture", 24, 40, F["5x7"], [[10, 10, 30, 20]], [1], [1000], [0.75], NAMES, scale=8)
    c("plate wider and taller than the picture", 18, 262, F["8x16 random"], [[100, 9, 130, 15], [5, 5, 9, 9]], [4, 1],
      [999, 1], [0.5, 0.5], NAMES, scale=3)
    c("overlapping captions: the last wins", 40, 300, F["5x7"],
      [[20, 20, 60, 38], [24, 21, 60, 38], [22, 19, 70, 36], [60, 20, 90, 30], [21, 22, 50, 30]], [0, 124, 31, 2, 62],
      [0, 1, 2, 3, 4], [0.9, 0.8, 0.7, 0.6, 0.5], NAMES)
    c("overlapping captions: the last wins", 24, 40, F["5x7"], [[4, 12, 30, 20], [6, 13, 30, 20], [5, 11, 30, 20]],
      [124, 0, 93], [10, 11, 12], None, None, scale=2, t=1)
    c("skipped labels leave no plate", 40, 300, F["5x7"],
      [[20, 20, 60, 38], [80, 20, 120, 38], [NAN, 20, 180, 38], [200, NAN, 240, 38], [200, 20, NAN, 38], [200, 20, 240, NAN],
       [250, 20, 290, 38]], [-1, P, 3, 4, 5, 6, -2147483648], [1, 2, 3, 4, 5, 6, 7], [0.5] * 7, NAMES)
    c("dark and light plates", 40, 300, F["5x7"], [[10 + 36 * i, 20, 40 + 36 * i, 36] for i in range(8)],
      [0, 124, 1, 5, 25, 62, 118, 31], list(range(8)), None, None, scale=1)
    # the operands that may be absent
    boxes, labels, idents, scores = _mixed(10, 40, 300, seed=77)
    c("no idents", 40, 300, F["5x7"], boxes, labels, None, scores, NAMES, scale=2)
    c("no scores", 40, 300, F["5x7"], boxes, labels, idents, None, NAMES, scale=2)
    c("no names", 40, 300, F["5x7"], boxes, labels, idents, scores, None, scale=2)
    c("only names", 40, 300, F["5x7"], boxes, labels, None, None, NAMES, scale=2)
    c("no operand at all: nothing is drawn", 40, 300, F["5x7"], boxes, labels, None, None, None, scale=2)
    c("empty names and absent idents: nothing is drawn", 24, 40, F["5x7"], [[5, 12, 30, 20], [8, 14, 30, 20]], [3, 3],
      [-1, -5], None, NAMES)
    c("a short name table and a small palette", 24, 40, F["5x7"], [[5, 12, 30, 20], [2, 20, 30, 23], [20, 12, 30, 20]],
      [0, 1, 2], [4, 5, 6], [0.25, 0.5, 0.75], name_table(["ab"]), palette=PALETTE[[124, 0]].copy())
    # the number of labels: none, one, more than one staging round, a full stage
    for n in (0, 1, 257, 1024):
        for H, W in ((18, 262), (40, 300)):
            boxes, labels, idents, scores = _mixed(n, H, W, seed=n + H)
            c(f"{n} labels", H, W, F["5x7"], boxes, labels, np.arange(n), None, None, scale=1 if H == 40 else 2, t=1, seed=n)
    boxes, labels, idents, scores = _mixed(1024, 24, 40, seed=4)
    c("1024 labels on one tile, long texts", 24, 40, F["5x7"], boxes, labels % len(NAME_LIST), idents, scores, NAMES, seed=5)
    # two samples with different contents
    for H, W in SIZES:
        b0, b1 = _mixed(9, H, W, seed=W), _mixed(9, H, W, seed=W + 1)
        c("two samples", H, W, F["5x7"], *(np.stack([x, y]) for x, y in zip(b0, b1)), NAMES, B=2, scale=1 if H < 40 else 2,
          seed=H)
    names = [case["name"] for case in out]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return out
