"""Looking at frames and boxes (reference future_od/utils/visualization.py, same names): the annotated frame of each
sample as an 8-bit RGB picture with box outlines, written as PNG.

The reference copies the whole normalised f32 clip to the host, draws with a Python loop over boxes and encodes with
torchvision.  Here a clip that lives on the GPU is rendered there by one launch (`render` -> ops.render_boxes,
include/fod_ext.h: fod_render_boxes) and only the finished uint8 picture crosses to the host; the PNG is written with
zlib and struct.  `draw_boxes` is the per-sample CPU form and the definition of the kernel's map, the way
datasets.transforms.photometric is for the photometric kernel; `render` on CPU tensors is built on it and gives the
kernel's bytes.

`render_attention` blends the attention maps that `predict(attention=True)` returns over the past frames they belong to
(reference demo.ipynb: F.interpolate of every query's map to full size, matplotlib on the host): one launch for all
pictures of a device clip (ops.render_attention, include/fod_ext.h: fod_render_attention), a torch form with the same
bytes for CPU tensors.

Captions (`Captions`, the `captions=` argument of `render` and `render_detections`) write a box's index, class name and
score on a plate above it (reference demo.ipynb: cv2.putText of every detection's index; visualize_wandb: "<idx>
<category>" and the score): the text is composed and rasterised on the device by one more launch (ops.render_labels,
include/fod_ext.h: fod_render_labels), so neither scores nor labels are read back; `label_text` and `draw_labels` are
the CPU form with the same bytes, `FONT_5X7` the font.

Not built: captions that avoid each other or stay inside their box, anti-aliased or proportional fonts, text that is
not ASCII, text in `render_attention`'s overlays, filled or alpha-blended boxes, a thickness per box, bf16 sources, PNG
compression tuning, drawing every frame of a clip to disk."""
import copy
import os
import struct
import zlib

import torch

_LEVELS = (0.0, 0.25, 0.5, 0.75, 1.0)
# f32 [125, 3]: entry a*25 + b*5 + c is (lv[c], lv[b], lv[a]) -- red runs fastest
COLOURS = torch.tensor([[_LEVELS[c], _LEVELS[b], _LEVELS[a]] for a in range(5) for b in range(5) for c in range(5)],
                       dtype=torch.float32)
PIXEL_MEAN, PIXEL_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)        # ImageNet's, as the loaders normalise


def revert_imagenet_normalization(sample):
    """sample [..., 3, H, W], normalised -> 0..1 scale: sample * std + mean (product and sum each rounded to f32)."""
    mean = torch.tensor(PIXEL_MEAN, dtype=torch.float32, device=sample.device).view(3, 1, 1)
    std = torch.tensor(PIXEL_STD, dtype=torch.float32, device=sample.device).view(3, 1, 1)
    return sample * std + mean


def to_bytes(values):
    """Float values on the 0..1 scale -> uint8: v * 255 truncated towards zero and clamped to 0..255; a product that is
    not finite gives 0.  (The reference's `.byte()` of an out-of-range float is undefined.)"""
    w = values * 255
    w = torch.where(torch.isfinite(w), w, torch.zeros_like(w))
    return w.clamp(0, 255).to(torch.uint8)


def draw_boxes(image, boxes, colours, thickness=3):
    """Outlines of `boxes` f32 [N, 4] (xyxy pixels) in `colours` [N, 3] on the float image [3, H, W], in place and
    returned.  A painter's loop: later boxes cover earlier ones.  With t = thickness, in f32 and then truncated:
        Lf = trunc(min(max(x1, t), W - t))   Rt = trunc(min(max(x2, t), W - t))
        Tp = trunc(min(max(y1, t), H - t))   Bt = trunc(min(max(y2, t), H - t))
    and four bars, rows x columns:
        left    [Tp - t, Bt)     x [Lf - t, Lf)        bottom  [Bt, Bt + t)     x [Lf - t, Rt)
        right   [Tp, Bt + t)     x [Rt, Rt + t)        top     [Tp - t, Tp)     x [Lf, Rt + t)
    An empty range holds nothing, so a reversed or collapsed box draws the bars that remain; the clamps keep every bar
    inside the image.  A box with a NaN coordinate is skipped (the reference raises on it)."""
    _, H, W = image.shape
    t = int(thickness)
    if t < 1 or H < 2 * t or W < 2 * t:
        raise ValueError(f"draw_boxes: a {H}x{W} image does not hold bars of thickness {thickness}")
    boxes = boxes.detach().to(torch.float32)
    for n in range(boxes.shape[0]):
        if bool(torch.isnan(boxes[n]).any()):
            continue
        Lf = int(boxes[n, 0].clamp(t, W - t))
        Tp = int(boxes[n, 1].clamp(t, H - t))
        Rt = int(boxes[n, 2].clamp(t, W - t))
        Bt = int(boxes[n, 3].clamp(t, H - t))
        colour = colours[n].to(image.dtype).view(3, 1, 1)
        image[:, Tp - t:Bt, Lf - t:Lf] = colour
        image[:, Bt:Bt + t, Lf - t:Rt] = colour
        image[:, Tp:Bt + t, Rt:Rt + t] = colour
        image[:, Tp - t:Tp, Lf:Rt + t] = colour
    return image


_DEVICE_CONSTANTS = {}


def _device_constants(device):
    """(COLOURS as bytes, mean, std) on `device`, made once."""
    hit = _DEVICE_CONSTANTS.get(device)
    if hit is None:
        hit = _DEVICE_CONSTANTS[device] = (to_bytes(COLOURS).to(device),
                                           torch.tensor(PIXEL_MEAN, dtype=torch.float32, device=device),
                                           torch.tensor(PIXEL_STD, dtype=torch.float32, device=device))
    return hit


# ---- captions: the text a box carries, a 5x7 font, the CPU form of include/fod_ext.h: fod_render_labels ------------------
LABEL_MAX_CHARS = 32                     # the text limit include/fod_ext.h states for fod_render_labels

# The glyphs of the codes 32..126, seven rows of five columns each, top row first (profiles/font_5x7.txt shows them
# enlarged; tools/font_art.py writes that file).  Drawn for this project.
_GLYPHS = (
    "..... ..... ..... ..... ..... ..... .....",  # space
    "..#.. ..#.. ..#.. ..#.. ..#.. ..... ..#..",  # !
    ".#.#. .#.#. .#.#. ..... ..... ..... .....",  # "
    ".#.#. .#.#. ##### .#.#. ##### .#.#. .#.#.",  # #
    "..#.. .#### #.#.. .###. ..#.# ####. ..#..",  # $
    "##... ##..# ...#. ..#.. .#... #..## ...##",  # %
    ".##.. #..#. #.#.. .#... #.#.# #..#. .##.#",  # &
    "..#.. ..#.. ..#.. ..... ..... ..... .....",  # '
    "...#. ..#.. .#... .#... .#... ..#.. ...#.",  # (
    ".#... ..#.. ...#. ...#. ...#. ..#.. .#...",  # )
    "..... ..#.. #.#.# .###. #.#.# ..#.. .....",  # *
    "..... ..#.. ..#.. ##### ..#.. ..#.. .....",  # +
    "..... ..... ..... ..... .##.. ..#.. .#...",  # ,
    "..... ..... ..... ##### ..... ..... .....",  # -
    "..... ..... ..... ..... ..... .##.. .##..",  # .
    "..... ....# ...#. ..#.. .#... #.... .....",  # /
    ".###. #...# #..## #.#.# ##..# #...# .###.",  # 0
    "..#.. .##.. ..#.. ..#.. ..#.. ..#.. .###.",  # 1
    ".###. #...# ....# ...#. ..#.. .#... #####",  # 2
    "##### ...#. ..#.. ...#. ....# #...# .###.",  # 3
    "...#. ..##. .#.#. #..#. ##### ...#. ...#.",  # 4
    "##### #.... ####. ....# ....# #...# .###.",  # 5
    "..##. .#... #.... ####. #...# #...# .###.",  # 6
    "##### ....# ...#. ..#.. .#... .#... .#...",  # 7
    ".###. #...# #...# .###. #...# #...# .###.",  # 8
    ".###. #...# #...# .#### ....# ...#. .##..",  # 9
    "..... .##.. .##.. ..... .##.. .##.. .....",  # :
    "..... .##.. .##.. ..... .##.. ..#.. .#...",  # ;
    "...#. ..#.. .#... #.... .#... ..#.. ...#.",  # <
    "..... ..... ##### ..... ##### ..... .....",  # =
    ".#... ..#.. ...#. ....# ...#. ..#.. .#...",  # >
    ".###. #...# ....# ...#. ..#.. ..... ..#..",  # ?
    ".###. #...# ....# .##.# #.#.# #.#.# .###.",  # @
    ".###. #...# #...# #...# ##### #...# #...#",  # A
    "####. #...# #...# ####. #...# #...# ####.",  # B
    ".###. #...# #.... #.... #.... #...# .###.",  # C
    "###.. #..#. #...# #...# #...# #..#. ###..",  # D
    "##### #.... #.... ####. #.... #.... #####",  # E
    "##### #.... #.... ####. #.... #.... #....",  # F
    ".###. #...# #.... #.### #...# #...# .####",  # G
    "#...# #...# #...# ##### #...# #...# #...#",  # H
    ".###. ..#.. ..#.. ..#.. ..#.. ..#.. .###.",  # I
    "..### ...#. ...#. ...#. ...#. #..#. .##..",  # J
    "#...# #..#. #.#.. ##... #.#.. #..#. #...#",  # K
    "#.... #.... #.... #.... #.... #.... #####",  # L
    "#...# ##.## #.#.# #.#.# #...# #...# #...#",  # M
    "#...# #...# ##..# #.#.# #..## #...# #...#",  # N
    ".###. #...# #...# #...# #...# #...# .###.",  # O
    "####. #...# #...# ####. #.... #.... #....",  # P
    ".###. #...# #...# #...# #.#.# #..#. .##.#",  # Q
    "####. #...# #...# ####. #.#.. #..#. #...#",  # R
    ".#### #.... #.... .###. ....# ....# ####.",  # S
    "##### ..#.. ..#.. ..#.. ..#.. ..#.. ..#..",  # T
    "#...# #...# #...# #...# #...# #...# .###.",  # U
    "#...# #...# #...# #...# #...# .#.#. ..#..",  # V
    "#...# #...# #...# #.#.# #.#.# #.#.# .#.#.",  # W
    "#...# #...# .#.#. ..#.. .#.#. #...# #...#",  # X
    "#...# #...# #...# .#.#. ..#.. ..#.. ..#..",  # Y
    "##### ....# ...#. ..#.. .#... #.... #####",  # Z
    ".###. .#... .#... .#... .#... .#... .###.",  # [
    "..... #.... .#... ..#.. ...#. ....# .....",  # \
    ".###. ...#. ...#. ...#. ...#. ...#. .###.",  # ]
    "..#.. .#.#. #...# ..... ..... ..... .....",  # ^
    "..... ..... ..... ..... ..... ..... #####",  # _
    ".#... ..#.. ...#. ..... ..... ..... .....",  # `
    "..... ..... .###. ....# .#### #...# .####",  # a
    "#.... #.... #.##. ##..# #...# #...# ####.",  # b
    "..... ..... .###. #.... #.... #...# .###.",  # c
    "....# ....# .##.# #..## #...# #...# .####",  # d
    "..... ..... .###. #...# ##### #.... .###.",  # e
    "..##. .#..# .#... ###.. .#... .#... .#...",  # f
    "..... .#### #...# #...# .#### ....# .###.",  # g
    "#.... #.... #.##. ##..# #...# #...# #...#",  # h
    "..#.. ..... .##.. ..#.. ..#.. ..#.. .###.",  # i
    "...#. ..... ..##. ...#. ...#. #..#. .##..",  # j
    "#.... #.... #..#. #.#.. ##... #.#.. #..#.",  # k
    ".##.. ..#.. ..#.. ..#.. ..#.. ..#.. .###.",  # l
    "..... ..... ##.#. #.#.# #.#.# #...# #...#",  # m
    "..... ..... #.##. ##..# #...# #...# #...#",  # n
    "..... ..... .###. #...# #...# #...# .###.",  # o
    "..... ####. #...# #...# ####. #.... #....",  # p
    "..... .#### #...# #...# .#### ....# ....#",  # q
    "..... ..... #.##. ##..# #.... #.... #....",  # r
    "..... ..... .#### #.... .###. ....# ####.",  # s
    ".#... .#... ###.. .#... .#... .#..# ..##.",  # t
    "..... ..... #...# #...# #...# #..## .##.#",  # u
    "..... ..... #...# #...# #...# .#.#. ..#..",  # v
    "..... ..... #...# #...# #.#.# #.#.# .#.#.",  # w
    "..... ..... #...# .#.#. ..#.. .#.#. #...#",  # x
    "..... #...# #...# #...# .#### ....# .###.",  # y
    "..... ..... ##### ...#. ..#.. .#... #####",  # z
    "...#. ..#.. ..#.. .#... ..#.. ..#.. ...#.",  # {
    "..#.. ..#.. ..#.. ..#.. ..#.. ..#.. ..#..",  # |
    ".#... ..#.. ..#.. ...#. ..#.. ..#.. .#...",  # }
    "..... ..... .#... #.#.# ...#. ..... .....",  # ~
)
# uint8 [95, 7]: one byte per glyph row, column col in bit 7 - col (the glyph in bits 7..3, the low three bits zero)
FONT_5X7 = torch.tensor([[sum(128 >> col for col, mark in enumerate(row) if mark == "#") for row in glyph.split()]
                         for glyph in _GLYPHS], dtype=torch.uint8)


def encode_names(names):
    """Class names -> the name table the captions read, uint8 [P, stride]: row i holds the bytes of names[i] (a list,
    or a dict {class id: name} as the loaders' category_dict; an id that is missing gives an empty row), cut at
    LABEL_MAX_CHARS and padded with 0; stride is the longest row's length (at least 1)."""
    if isinstance(names, dict):
        names = [names.get(i, "") for i in range(max(names, default=-1) + 1)]
    rows = [str(name).encode("utf-8")[:LABEL_MAX_CHARS] for name in names]
    stride = max([len(row) for row in rows] + [1])
    table = torch.zeros((max(len(rows), 1), stride), dtype=torch.uint8)
    for i, row in enumerate(rows):
        table[i, :len(row)] = torch.tensor(list(row), dtype=torch.uint8)
    return table


def label_text(ident, label, score, names):
    """The bytes of one caption (include/fod_ext.h, fod_render_labels): the parts that are present joined by one space,
    cut at LABEL_MAX_CHARS.  `ident` (None, or an integer: present from 0 on) gives its decimal digits; `names` (None, or
    uint8 [n_names, stride]) gives the bytes of row `label` up to its first 0 where 0 <= label < n_names; `score` (None,
    or a number: present unless NaN) gives two digits of min(99, max(0, trunc(score * 100))), the product in f32."""
    parts = []
    if ident is not None and int(ident) >= 0:
        parts.append(str(int(ident)).encode())
    if names is not None and 0 <= int(label) < names.shape[0]:
        parts.append(bytes(names[int(label)].tolist()).split(b"\0")[0])
    if score is not None:
        product = torch.as_tensor(score).detach().to("cpu", torch.float32) * torch.tensor(100.0, dtype=torch.float32)
        if not bool(torch.isnan(product)):
            parts.append(b"%02d" % int(product.clamp(0.0, 99.0)))
    return b" ".join(parts)[:LABEL_MAX_CHARS]


def draw_labels(picture, boxes, labels, idents=None, scores=None, names=None, palette=None, font=FONT_5X7,
                font_first=32, font_width=5, scale=2, thickness=3):
    """Captions of one sample on the uint8 picture [H, W, 3] that holds its outlines, in place and returned: the CPU
    form of fod_render_labels (include/fod_ext.h states the map).  boxes f32 [N, 4], labels [N], idents [N] / scores
    [N] / names uint8 [n_names, stride] or None, palette uint8 [P, 3] (None: COLOURS as bytes), font uint8 [G, FH] with
    glyphs `font_width` columns wide for the codes from `font_first` on.  A painter's loop: label n's text on an opaque
    plate of its class colour above its box (inside it at the top border), black or white ink by the plate's
    brightness; later plates cover earlier ones."""
    H, W, _ = picture.shape
    t, s, FW = int(thickness), int(scale), int(font_width)
    G, FH = font.shape
    if t < 1 or H < 2 * t or W < 2 * t:
        raise ValueError(f"draw_labels: a {H}x{W} picture does not hold bars of thickness {thickness}")
    if not (1 <= s <= 8 and 1 <= FW <= 8 and 1 <= FH <= 16 and font_first >= 0 and font_first + G <= 256):
        raise ValueError(f"draw_labels: scale {s} (1..8), a {FW}x{FH} font cell (1..8 x 1..16) or {G} glyphs from code "
                         f"{font_first} on (inside 0..255)")
    palette = to_bytes(COLOURS) if palette is None else palette
    boxes = boxes.detach().to(torch.float32)
    cw, Hp = FW + 1, (FH + 2) * s
    shifts = 7 - torch.arange(FW)
    for n in range(boxes.shape[0]):
        label = int(labels[n])
        if not 0 <= label < palette.shape[0] or bool(torch.isnan(boxes[n]).any()):
            continue
        text = label_text(None if idents is None else idents[n], label, None if scores is None else scores[n], names)
        if not text:
            continue
        Wp = (len(text) * cw + 1) * s
        Lf, Tp = int(boxes[n, 0].clamp(t, W - t)), int(boxes[n, 1].clamp(t, H - t))
        x0, y0 = Lf - t, Tp - t - Hp
        if y0 < 0:
            y0 = Tp
        x0, y0 = max(min(x0, W - Wp), 0), max(min(y0, H - Hp), 0)
        mask = torch.zeros((FH + 2, len(text) * cw + 1), dtype=torch.bool)
        for i, code in enumerate(text):
            if font_first <= code < font_first + G:
                rows = font[code - font_first].to(torch.int64)
                mask[1:FH + 1, 1 + i * cw:1 + i * cw + FW] = (rows[:, None] >> shifts[None, :] & 1).bool()
        mask = mask.repeat_interleave(s, dim=0).repeat_interleave(s, dim=1)[:H - y0, :W - x0]
        plate = palette[label].to(torch.int64)
        dark = int(299 * plate[0] + 587 * plate[1] + 114 * plate[2]) < 128000
        ink = torch.full((3,), 255 if dark else 0, dtype=torch.uint8)
        picture[y0:y0 + Hp, x0:x0 + Wp] = torch.where(mask[..., None], ink, plate.to(torch.uint8))
    return picture


class Captions:
    """What `render` / `render_detections` write on a box, and how.  names: the class names (a list, a dict
    {class id: name}, or an `encode_names` table) or None; ident: None, "slot" -- the label's position n in its sample,
    which for `render_detections` is the slot that `render_attention(..., slot=n)` takes --, "query" (`render_detections`
    only: det["query"]) or an integer tensor [B, N]; scores: False, True (`render_detections` only: det["scores"]) or a
    float tensor [B, N]; scale: 1..8, the size of a font pixel; font: uint8 [G, FH] for the codes from `font_first`
    on, `font_width` columns wide.  The tables are copied to a device once, at the first picture rendered there."""

    def __init__(self, names=None, ident=None, scores=False, scale=2, font=FONT_5X7, font_first=32, font_width=5):
        if not (ident is None or isinstance(ident, torch.Tensor) or ident in ("slot", "query")):
            raise ValueError(f"Captions: ident is None, 'slot', 'query' or a tensor, not {ident!r}")
        if not (isinstance(scores, (bool, torch.Tensor)) or scores is None):
            raise ValueError(f"Captions: scores is a flag or a tensor, not {scores!r}")
        if names is not None and not isinstance(names, torch.Tensor):
            names = encode_names(names)
        self.names, self.ident, self.scores = names, ident, (False if scores is None else scores)
        self.scale, self.font, self.font_first, self.font_width = int(scale), font, int(font_first), int(font_width)
        self._on = {}

    def replace(self, ident, scores):
        """A copy with another `ident` and `scores`; it shares the tables already on a device."""
        other = copy.copy(self)
        other.ident, other.scores = ident, scores
        return other

    def tables(self, device):
        """(names or None, font) on `device`, made once."""
        hit = self._on.get(device)
        if hit is None:
            hit = self._on[device] = (None if self.names is None else self.names.to(device, torch.uint8).contiguous(),
                                      self.font.to(device, torch.uint8).contiguous())
        return hit

    def operands(self, labels, det=None):
        """(idents or None, scores or None) for `labels` [B, N], on its device; `det`: what predict() returned."""
        ident, scores = self.ident, self.scores
        if isinstance(ident, str):
            if ident == "query":
                if det is None:
                    raise ValueError("Captions: ident='query' needs the detections of render_detections")
                ident = det["query"]
            else:
                ident = torch.arange(labels.shape[1], dtype=torch.int32, device=labels.device)[None].expand(labels.shape)
        if scores is True:
            if det is None:
                raise ValueError("Captions: scores=True needs the detections of render_detections")
            scores = det["scores"]
        elif scores is False:
            scores = None
        for name, t in (("ident", ident), ("scores", scores)):
            if t is not None and tuple(t.shape) != tuple(labels.shape):
                raise ValueError(f"Captions: {name} {tuple(t.shape)} is not {tuple(labels.shape)}, one per label")
        return ident, scores


def render(video, boxes, labels, frame_idx=None, thickness=3, palette=COLOURS, captions=None):
    """The frame `frame_idx[b]` (None: frame 0; negative: from the end; clamped into the clip) of every sample of
    `video` [B, L, 3, H, W] -- f32 normalised, or raw uint8 -- with the outlines of `boxes` [B, N, 4] (xyxy pixels)
    -> uint8 [B, H, W, 3] on the clip's device.  Box n is drawn where 0 <= labels[b, n] < len(palette) (and no
    coordinate is NaN) in the colour palette[label]; `palette` is float [P, 3] on the 0..1 scale and becomes bytes by
    `to_bytes` (COLOURS: 0, 63, 127, 191, 255).  `labels` may be i64.  A device clip is one launch of ops.render_boxes;
    CPU tensors go through `draw_boxes` per sample and give the same bytes.  `captions` (a `Captions`, or None for
    outlines only) writes its text above every drawn box: one more launch (ops.render_labels) on a device clip,
    `draw_labels` on CPU tensors, the same bytes."""
    return _render(video, boxes, labels, frame_idx, thickness, palette, captions, None)


def _render(video, boxes, labels, frame_idx, thickness, palette, captions, det):
    if video.dim() != 5 or video.shape[2] != 3 or video.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"render: video must be f32 or uint8 [B, L, 3, H, W], got {video.dtype} {tuple(video.shape)}")
    B, L = video.shape[:2]
    idents = scores = None
    if captions is not None:
        idents, scores = captions.operands(labels, det)
    if video.is_cuda:
        from future_od.native import ops
        colours, mean, std = _device_constants(video.device)
        if palette is not COLOURS:
            colours = to_bytes(palette.to(video.device, torch.float32)).contiguous()
        if frame_idx is not None:
            frame_idx = frame_idx.to(video.device, torch.int32).contiguous()
        boxes = boxes.to(video.device, torch.float32).contiguous()
        labels = labels.to(video.device, torch.int32).contiguous()
        pictures = ops.render_boxes(video, boxes, labels, frame_idx=frame_idx, mean=mean, std=std, palette=colours,
                                    thickness=thickness)
        if captions is None:
            return pictures
        names, font = captions.tables(video.device)
        return ops.render_labels(pictures, boxes, labels,
                                 idents=None if idents is None else idents.to(video.device, torch.int32).contiguous(),
                                 scores=None if scores is None else scores.to(video.device, torch.float32).contiguous(),
                                 names=names, palette=colours, font=font, font_first=captions.font_first,
                                 font_width=captions.font_width, scale=captions.scale, thickness=thickness)
    u8 = video.dtype == torch.uint8
    palette = palette.to(torch.float32)
    colours = to_bytes(palette).to(torch.float32) if u8 else palette
    out = []
    for b in range(B):
        f = 0 if frame_idx is None else int(frame_idx[b])
        f = min(max(f + L if f < 0 else f, 0), L - 1)
        keep = (labels[b] >= 0) & (labels[b] < palette.shape[0])
        image = video[b, f].to(torch.float32) if u8 else revert_imagenet_normalization(video[b, f])
        image = draw_boxes(image, boxes[b][keep], colours[labels[b][keep].long()], thickness)
        picture = (image.to(torch.uint8) if u8 else to_bytes(image)).permute(1, 2, 0).contiguous()
        if captions is not None:
            draw_labels(picture, boxes[b], labels[b], None if idents is None else idents[b],
                        None if scores is None else scores[b], captions.names, to_bytes(palette), captions.font,
                        captions.font_first, captions.font_width, captions.scale, thickness)
        out.append(picture)
    return torch.stack(out).contiguous()


def render_detections(video, det, min_score=0.5, frame_idx=None, thickness=3, palette=COLOURS, captions=None):
    """`render` of what `predict()` returns ({"scores" [B, K], "labels" [B, K], "boxes" [B, K, 4], "count" [B]}): the
    slots that hold a detection (index < count) with a score of at least `min_score`.  A few tiny torch ops on the
    tensors' device, no read-back.  With `captions`, ident="slot" numbers every box with its position k in `det` --
    what `render_attention(..., slot=k)` takes --, ident="query" prints det["query"], scores=True det["scores"]."""
    scores, labels = det["scores"], det["labels"]
    slot = torch.arange(labels.shape[1], device=labels.device)
    hidden = (scores < min_score) | (slot[None, :] >= det["count"][:, None])
    return _render(video, det["boxes"], labels.masked_fill(hidden, -1), frame_idx, thickness, palette, captions, det)


def track_colour_index(det, min_hits=1, palette=COLOURS):
    """What `render_tracks` hands `render` as labels, i32 [B, K]: track % len(palette) for the rows that carry an
    identity seen at least `min_hits` times, -1 (not drawn) for every other row."""
    track, hits = det["track"], det["track_hits"]
    return torch.where((track >= 0) & (hits >= min_hits), track % palette.shape[0], torch.full_like(track, -1))


def render_tracks(video, det, min_hits=1, frame_idx=None, thickness=3, palette=COLOURS, captions=None):
    """`render` of what `DetectionTracker.update` returns: the rows with an identity (track >= 0) that has been seen in
    at least `min_hits` calls, in the colour palette[track % len(palette)] -- the colour follows the OBJECT from picture
    to picture, not the class.  It is `render` with `track_colour_index` as the labels: no launch of its own, and CPU
    tensors give the same bytes.  With `captions` the number on a box is its identity (ident = det["track"], whatever the
    Captions' own `ident` says); scores=True prints det["scores"].  A Captions with `names` is refused: names go by the
    label, which here is the colour index."""
    if captions is not None:
        if captions.names is not None:
            raise ValueError("render_tracks: captions with names would print the name of the colour index, not of the class")
        captions = captions.replace(det["track"], captions.scores)
    return _render(video, det["boxes"], track_colour_index(det, min_hits, palette), frame_idx, thickness, palette,
                   captions, det)


# uint8 [256, 3], a diverging blue - white - red ramp by an integer rule: entry i is (2i, 2i, 255) for i <= 127 and
# (255, 2(255 - i), 2(255 - i)) for i >= 128 -- blue at 0, (254, 254, 255) | (255, 254, 254) in the middle, red at 255.
# (Not matplotlib's `coolwarm`, which the reference's notebook uses: same idea, other numbers.)
ATTENTION_LUT = torch.tensor([[2 * i, 2 * i, 255] if i <= 127 else [255, 2 * (255 - i), 2 * (255 - i)] for i in range(256)],
                             dtype=torch.uint8)


def _taps(n_out, n_in):
    """Bilinear source rows of `n_out` destination rows over `n_in` (F.interpolate's coordinate, align_corners=False),
    every step one f32 operation: f = max((d + 0.5) * (n_in / n_out) - 0.5, 0), i0 = min(trunc(f), n_in - 1),
    i1 = min(i0 + 1, n_in - 1), w1 = f - i0, w0 = 1 - w1."""
    ratio = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)
    f = (((torch.arange(n_out, dtype=torch.float32) + 0.5) * ratio) - 0.5).clamp_min(0.0)
    i0 = f.to(torch.int64).clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    w1 = f - i0.to(torch.float32)
    return i0, i1, 1.0 - w1, w1


def overlay_map(background, amap, colour_scale, gain=50.0, max_alpha=0.4, lut=ATTENTION_LUT):
    """One picture of `render_attention` on the CPU and the definition of the kernel's map: `background` uint8 [3, H, W],
    `amap` f32 [h, w] -> uint8 [H, W, 3].  With a = the bilinear sample of the map (top = m[y0,x0] * wx0 + m[y0,x1] * wx1,
    bot likewise on row y1, a = top * wy0 + bot * wy1):
        alpha = min(max(a * gain, 0), max_alpha)      colour = lut[trunc(min(max(a * colour_scale, 0), 1) * 255)]
        byte = trunc(min(max(bg * (1 - alpha) + colour * alpha, 0), 255))
    every step one f32 operation; max(v, 0) of a NaN is 0; where a is not finite the background stays."""
    f32 = torch.float32
    _, H, W = background.shape
    h, w = amap.shape
    y0, y1, wy0, wy1 = _taps(H, h)
    x0, x1, wx0, wx1 = _taps(W, w)
    m = amap.to(f32)
    top = m[y0][:, x0] * wx0 + m[y0][:, x1] * wx1
    bot = m[y1][:, x0] * wx0 + m[y1][:, x1] * wx1
    a = top * wy0[:, None] + bot * wy1[:, None]
    zero = torch.zeros((), dtype=f32)
    alpha = a * torch.tensor(float(gain), dtype=f32)
    alpha = torch.minimum(torch.where(alpha >= 0, alpha, zero), torch.tensor(float(max_alpha), dtype=f32))
    level = a * torch.as_tensor(colour_scale, dtype=f32)
    level = torch.minimum(torch.where(level >= 0, level, zero), torch.ones((), dtype=f32)) * 255.0
    colour = lut.to(f32)[level.to(torch.int64)]                                   # [H, W, 3]
    bg = background.permute(1, 2, 0).to(f32)
    mixed = bg * (1.0 - alpha)[..., None] + colour * alpha[..., None]
    mixed = torch.where(torch.isfinite(a)[..., None], mixed, bg)
    return mixed.clamp(0, 255).to(torch.uint8)


_LUT_ON = {}


def render_attention(video, attention, frames, slot, gain=50.0, max_alpha=0.4, lut=ATTENTION_LUT):
    """The attention maps of ONE detection per sample over the past frames they look at -> uint8 [B, J, H, W, 3] on the
    clip's device.  `video` [B, L, 3, H, W] f32 normalised or raw uint8; `attention` f32 [B, K, J, h, w] and `frames`
    i32 [J] as `predict(attention=True)` returns them ("attention", "attention_frames": picture j is clip frame
    frames[j]; negative counts from the end, then clamped); `slot`: which of the K detections, an int or i32 [B].
    Per picture the map is upsampled bilinearly, coloured through `lut` (uint8 [256, 3]) after scaling by 1 / its
    maximum, and blended with alpha = min(map * gain, max_alpha) (`overlay_map` states every step; the reference's
    notebook uses 50 and 0.4).  A device clip is one launch of ops.render_attention; CPU tensors go through
    `overlay_map` per picture and give the same bytes."""
    if video.dim() != 5 or video.shape[2] != 3 or video.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"render_attention: video must be f32 or uint8 [B, L, 3, H, W], got {video.dtype} "
                         f"{tuple(video.shape)}")
    B, L = video.shape[:2]
    if attention.dim() != 5 or attention.shape[0] != B:
        raise ValueError(f"render_attention: attention must be [B, K, J, h, w] for {B} samples, got {tuple(attention.shape)}")
    if not 0.0 <= float(max_alpha) <= 1.0:
        raise ValueError(f"render_attention: max_alpha {max_alpha} outside [0, 1]")
    K, J = attention.shape[1:3]
    attention = attention.to(video.device, torch.float32)
    if isinstance(slot, int):
        maps = attention[:, slot]                                                  # a view: no copy
    else:
        maps = attention[torch.arange(B, device=video.device), slot.to(video.device, torch.int64)]
    frames = torch.as_tensor(frames).to(video.device, torch.int32).reshape(J)
    # matplotlib's auto-normalisation: the colour runs up to the map's maximum (an all-zero map stays at lut[0])
    colour_scale = 1.0 / maps.amax(dim=(2, 3)).clamp_min(1e-30)
    if video.is_cuda:
        from future_od.native import ops
        _, mean, std = _device_constants(video.device)
        key = (video.device, id(lut))
        if key not in _LUT_ON:
            _LUT_ON[key] = (lut, lut.to(video.device).contiguous())       # (the table is kept: its id stays its own)
        return ops.render_attention(video, maps, frames[None].expand(B, J).contiguous(), colour_scale.contiguous(),
                                    mean=mean, std=std, lut=_LUT_ON[key][1], gain=gain, max_alpha=max_alpha)
    out = []
    for b in range(B):
        for j in range(J):
            f = int(frames[j])
            f = min(max(f + L if f < 0 else f, 0), L - 1)
            bg = video[b, f] if video.dtype == torch.uint8 else to_bytes(revert_imagenet_normalization(video[b, f]))
            out.append(overlay_map(bg, maps[b, j], colour_scale[b, j], gain, max_alpha, lut))
    return torch.stack(out).view(B, J, *out[0].shape).contiguous()


def _chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def write_png(img_hwc_uint8, path):
    """uint8 [H, W, 3] -> an 8-bit RGB PNG: non-interlaced, filter 0 on every line, one IDAT.  Creates the directory."""
    img = img_hwc_uint8.detach().cpu() if isinstance(img_hwc_uint8, torch.Tensor) else torch.as_tensor(img_hwc_uint8)
    if img.dim() != 3 or img.shape[2] != 3 or img.dtype != torch.uint8:
        raise ValueError(f"write_png: uint8 [H, W, 3], got {img.dtype} {tuple(img.shape)}")
    H, W, _ = img.shape
    lines = torch.cat([torch.zeros(H, 1, dtype=torch.uint8), img.reshape(H, 3 * W)], dim=1)    # the filter byte first
    data = (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))
            + _chunk(b"IDAT", zlib.compress(lines.contiguous().numpy().tobytes())) + _chunk(b"IEND", b""))
    if os.path.dirname(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(data)


def visualize(image, classes, boxes, fpath, BACKGROUND_CLASS):
    """image [3, H, W] normalised; classes float [M, C] (scores: best class, background below 0.5) or integer [M];
    boxes [M, 4] xyxy pixels or None.  Writes the picture to `fpath` and returns it, uint8 [H, W, 3] on the image's
    device."""
    print("Storing visualization at", fpath)
    if boxes is None:
        boxes, classes = image.new_zeros((0, 4), dtype=torch.float32), torch.zeros(0, dtype=torch.int64)
    elif classes.is_floating_point():
        scores, classes = classes.max(dim=1)
        classes = classes.masked_fill(scores < 0.5, BACKGROUND_CLASS)
    classes = classes.to(boxes.device)
    keep = classes != BACKGROUND_CLASS
    picture = render(image[None, None], boxes[keep][None], classes[keep][None])[0]
    write_png(picture, fpath)
    return picture


def _pixel_box(box, class_id):
    x1, y1, x2, y2 = (int(v) for v in box.round())
    return {"position": {"minX": x1, "maxX": x2, "minY": y1, "maxY": y2}, "domain": "pixel", "class_id": class_id}


def wandb_box_data(background_class, category_dict, pred_scores=None, pred_boxes=None, anno_classes=None,
                   anno_boxes=None, ignore_boxes=None):
    """The `boxes` argument of a wandb.Image, as the reference's visualize_wandb builds it: "predictions" (best class of
    pred_scores [M, C] where its score is above 0.1, captioned "<index> <category>"), "ground_truth" (anno_classes [N]
    other than the background class) and "ignore_regions"; positions are rounded pixel integers.  A pure function of
    host or device tensors; nothing of wandb is touched."""
    host = lambda t: t.detach().cpu().numpy()
    out = {}
    if pred_boxes is not None:
        scores, classes = pred_scores.max(dim=1)
        data = []
        for idx, (score, cls, box) in enumerate(zip(host(scores), host(classes), host(pred_boxes))):
            if score > 0.1:
                data.append({**_pixel_box(box, int(cls)), "scores": {"score": float(score)},
                             "box_caption": f"{idx} {category_dict[int(cls)]}"})
        out["predictions"] = {"box_data": data, "class_labels": category_dict}
    if anno_classes is not None:
        out["ground_truth"] = {"box_data": [_pixel_box(box, int(cls)) for cls, box in zip(host(anno_classes), host(anno_boxes))
                                            if cls != background_class],
                               "class_labels": category_dict}
    if ignore_boxes is not None:
        out["ignore_regions"] = {"box_data": [_pixel_box(box, 0) for box in host(ignore_boxes)],
                                 "class_labels": {0: "Ignore"}}
    return out


def visualize_wandb(image, background_class, category_dict, pred_scores=None, pred_boxes=None, anno_classes=None,
                    anno_boxes=None, ignore_boxes=None, model_mood=None):
    """wandb.Image of the frame [3, H, W] (normalised float, or raw uint8) on the 0..1 scale with `wandb_box_data`'s
    boxes; RuntimeError without wandb."""
    try:
        import wandb
    except ImportError:
        raise RuntimeError("visualize_wandb: the wandb package is not installed; `visualize` writes PNG files "
                           "without it") from None
    boxes = wandb_box_data(background_class, category_dict, pred_scores, pred_boxes, anno_classes, anno_boxes,
                           ignore_boxes)
    image = image.detach()
    picture = image.float() / 255 if image.dtype == torch.uint8 else revert_imagenet_normalization(image.float())
    picture = picture.cpu().numpy().transpose(1, 2, 0)
    return wandb.Image(picture, boxes=boxes, caption=model_mood)
