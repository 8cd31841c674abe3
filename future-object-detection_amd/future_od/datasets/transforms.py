"""Joint transforms of a clip and its boxes, with the class names and constructor arguments of the reference
(reference future_od/datasets/transforms.py; composed by its loaders, runs/_loader.py:30-35,45,74-79,89).

Every transform has two faces:

* `t(images, boxes, classes) -> (images, boxes, classes)`: the per-sample CPU form.  `images` is a float clip
  [L, 3, h, w], `boxes` [n, 4] are xyxy pixels, `classes` [n].  This is what a CPU dataset calls and what the device
  path is tested against.  Cropping is slicing, resizing is `F.interpolate(mode="bilinear", align_corners=False)`
  without antialiasing (what the reference's pinned torchvision does to tensors).
* `t.plan(h, w, rng) -> Plan`: draws the transform's random numbers and returns the GEOMETRY for a frame of that size
  -- one source rectangle, the output size, a flip flag -- plus the annotation steps.  The image half of a plan is one
  bilinear pass, which is what `fod_clip_crop_resize` executes on the device from the raw uint8 frames
  (future_od/utils/augment.py); the annotation half runs on the host (`Plan.annotate`).

Plannable is: crops (a rectangle inside a rectangle composes exactly), then at most one `JointResize`, then at most one
`JointHorizontalFlip`, with `SizeFilter` / no-ops anywhere; `RandomSelect` plans the branch it draws.  Anything else
would need a second resampling: `plan` raises ValueError naming the step, it never approximates.

`JointResize(..., antialias=True)` is opt-in (the reference's pinned torchvision does not antialias tensors; current
torchvision does by default): the CPU form passes `antialias=True` to `F.interpolate`, the plan carries the flag
(`Plan.antialias`) and the device half runs `fod_clip_crop_resize_aa`.  Geometry, annotations and draws do not change.

`JointPhotometricDistortion` is the colour half: per-pixel work, which commutes exactly with crops and flips but not
with resampling.  A plan carries at most one row of it (`Plan.photo`), drawn once per clip, and a `JointResize` may not
follow it; `fod_clip_crop_resize_photo` applies the row to the resampled pixels in the same pass.

Random numbers come from a `random.Random`-like `rng`; `rng=None` (and `__call__`) means Python's global `random`
module, so `random.seed(s); t(...)` and `t.plan(h, w, random.Random(s))` draw the same numbers.

Annotation rules (the reference's, quirks included): a crop subtracts (left, top, left, top), keeps a box iff
x0 <= width and y0 <= height and x1 >= 0 and y1 >= 0 (inclusive: a box that only touches the crop survives as a
degenerate one), then clamps to [0, width] x [0, height]; a resize multiplies by (new_w / old_w, new_h / old_h, ...);
a flip maps (x0, x1) -> (w - x1, w - x0); `SizeFilter` keeps area / (h * w) > min_size.  The sized crops use ONE scale
for both sides: int(h * scale), int(w * scale)."""
import random as _random
from abc import ABC, abstractmethod
from typing import List, Tuple

import torch
import torch.nn.functional as F


class ImageRemap:
    """uint8 0..255 -> float 0..1."""

    def __call__(self, tensor):
        return tensor.float() / 255


# ---- annotation steps: plain tuples, applied by ONE function for both faces -------------------------------------------
# ("crop", left, top, width, height) | ("resize", old_w, old_h, new_w, new_h) | ("flip", width)
# | ("size_filter", width, height, min_size)

def annotate(step, boxes, classes):
    """One annotation step on boxes [n, 4] (xyxy pixels, float) and classes [n]; returns new tensors."""
    kind = step[0]
    if kind == "crop":
        _, left, top, width, height = step
        boxes = boxes - torch.tensor([left, top, left, top], dtype=boxes.dtype)
        keep = (boxes[:, 0] <= width) & (boxes[:, 1] <= height) & (boxes[:, 2] >= 0) & (boxes[:, 3] >= 0)
        boxes, classes = boxes[keep], classes[keep]
        hi = torch.tensor([width, height, width, height], dtype=boxes.dtype)
        return torch.minimum(boxes.clamp(min=0), hi), classes
    if kind == "resize":
        _, old_w, old_h, new_w, new_h = step
        w_scale, h_scale = new_w / old_w, new_h / old_h
        return boxes * torch.tensor([w_scale, h_scale, w_scale, h_scale], dtype=boxes.dtype), classes
    if kind == "flip":
        width = step[1]
        return torch.stack([width - boxes[:, 2], boxes[:, 1], width - boxes[:, 0], boxes[:, 3]], dim=1), classes
    if kind == "size_filter":
        _, width, height, min_size = step
        area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
        keep = (area / (height * width)) > min_size
        return boxes[keep], classes[keep]
    raise ValueError(f"unknown annotation step {step!r}")


# ---- the photometric row: (delta, alpha, sat, hue, first), one per clip ------------------------------------------------
PHOTO_NEUTRAL = (0.0, 1.0, 1.0, 0.0, 0.0)


def sanitise_photo_row(row):
    """The row as the kernel uses it, in float32: a non-finite delta / alpha / sat / hue becomes its neutral value, then
    delta -> [-1, 1], alpha and sat -> [0, 4], hue -> hue - floor(hue); first counts as set unless it equals 0.
    -> (delta, alpha, sat, hue, first) as python floats that are float32 values, and a bool."""
    v = torch.tensor([float(x) for x in row], dtype=torch.float32)
    if v.shape != (5,):
        raise ValueError(f"a photometric row is (delta, alpha, sat, hue, first), got {tuple(row)!r}")
    v[:4] = torch.where(torch.isfinite(v[:4]), v[:4], torch.tensor(PHOTO_NEUTRAL[:4]))
    delta, alpha, sat = v[0].clamp(-1, 1), v[1].clamp(0, 4), v[2].clamp(0, 4)
    hue = v[3] - torch.floor(v[3])
    return float(delta), float(alpha), float(sat), float(hue), not bool(v[4] == 0)


def photometric(images, row):
    """The photometric map of include/fod_ext.h (fod_clip_crop_resize_photo, steps 1-5) on a float32 clip [..., 3, h, w]
    in 0..1, every step in float32: ONE row for all frames.  A neutral row returns `images` itself."""
    delta, alpha, sat, hue, first = sanitise_photo_row(row)
    hsv = sat != 1.0 or hue != 0.0
    if delta == 0.0 and alpha == 1.0 and not hsv:
        return images
    if images.dtype != torch.float32 or images.dim() < 3 or images.shape[-3] != 3:
        raise ValueError(f"the photometric map takes a float32 clip [..., 3, h, w], got {images.dtype} {tuple(images.shape)}")
    p = images + delta
    if first:
        p = p * alpha
    if hsv:
        r, g, b = p.clamp(0, 1).unbind(-3)
        v, m = torch.maximum(r, torch.maximum(g, b)), torch.minimum(r, torch.minimum(g, b))
        c = v - m
        grey = c == 0
        cs = torch.where(grey, torch.ones_like(c), c)                     # a safe divisor; grey pixels take the zeros
        s = torch.where(grey, torch.zeros_like(c), c / torch.where(grey, torch.ones_like(v), v))
        h6 = torch.where(v == r, torch.remainder((g - b) / cs, 6.0),
                         torch.where(v == g, (b - r) / cs + 2.0, (r - g) / cs + 4.0))
        h6 = torch.where(grey, torch.zeros_like(c), h6)
        s = (s * sat).clamp(max=1)
        h = h6 / 6.0 + hue
        h = h - torch.floor(h)

        def f(n):
            k = torch.fmod(n + 6.0 * h, 6.0)
            return v - v * s * torch.minimum(torch.minimum(k, 4.0 - k), torch.ones_like(k)).clamp(min=0)
        p = torch.stack([f(5.0), f(3.0), f(1.0)], dim=-3)
    if not first:
        p = p * alpha
    return p.clamp(0, 1)


class Plan:
    """Composed geometry of a joint transform for one frame size: `rect` = (top, left, height, width) in the source
    frame, `size` = (H, W) of the output, `flip`, and the annotation `steps` in the order they were composed."""

    def __init__(self, h, w):
        self.source = (int(h), int(w))
        self.rect = (0, 0, int(h), int(w))
        self.size = (int(h), int(w))
        self.flip = False
        self.steps = []
        self.photo = None                     # (delta, alpha, sat, hue, first) of a JointPhotometricDistortion, if any
        self.antialias = False                # the JointResize's flag: the image half is the antialiased pass
        self._resized = self._flip_seen = False

    def row(self):
        """(top, left, height, width, flip): a row of the `plans` operand of ops.clip_crop_resize."""
        return (*self.rect, int(self.flip))

    def photo_row(self):
        """(delta, alpha, sat, hue, first): a row of the `photo` operand of ops.clip_crop_resize_photo; the neutral row
        for a plan without a photometric step."""
        return PHOTO_NEUTRAL if self.photo is None else tuple(float(v) for v in self.photo)

    def annotate(self, boxes, classes):
        for step in self.steps:
            boxes, classes = annotate(step, boxes, classes)
        return boxes, classes

    def box_map(self):
        """(sx, sy, ox, oy): output-pixel coordinates back to source-frame pixels, x_src = x * sx + ox and y_src =
        y * sy + oy -- the inverse of `annotate` for boxes inside the rectangle.  A flip gives sx < 0: the caller
        re-orders the corners (detect.detect_select does)."""
        top, left, h, w = self.rect
        H, W = self.size
        if self.flip:
            return (-w / W, h / H, float(left + w), float(top))
        return (w / W, h / H, float(left), float(top))

    def __repr__(self):
        return f"Plan(rect={self.rect}, size={self.size}, flip={self.flip}, steps={self.steps})"


class JointTransform(ABC):
    @abstractmethod
    def __call__(self, images, boxes, classes) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Perform a joint transform."""

    @abstractmethod
    def _extend(self, plan: Plan, rng) -> None:
        """Draw this transform's random numbers from `rng` and compose it onto `plan`."""

    def plan(self, h, w, rng=None) -> Plan:
        plan = Plan(h, w)
        self._extend(plan, _random if rng is None else rng)
        return plan


class JointNoOpTransform(JointTransform):
    def __call__(self, images, boxes, classes):
        return images, boxes, classes

    def _extend(self, plan, rng):
        pass


class JointCompose(JointTransform):
    def __init__(self, transforms: List[JointTransform]):
        self.transforms = transforms

    def __call__(self, images, boxes, classes):
        for transform in self.transforms:
            images, boxes, classes = transform(images, boxes, classes)
        return images, boxes, classes

    def _extend(self, plan, rng):
        for transform in self.transforms:
            if not hasattr(transform, "_extend"):
                raise ValueError(f"{type(transform).__name__} cannot be planned: it does not describe its geometry")
            transform._extend(plan, rng)


class JointResize(JointTransform):
    """`antialias=True` (bilinear only; the default stays the reference's False) averages the whole source footprint of
    an output pixel, `F.interpolate(..., antialias=True)`: what the device pass does as `fod_clip_crop_resize_aa`."""

    def __init__(self, size: Tuple[int, int], interpolation: str = "bilinear", antialias: bool = False):
        self._size = [int(v) for v in size]
        self._interpolation = getattr(interpolation, "value", interpolation)
        self._antialias = bool(antialias)
        if self._antialias and self._interpolation != "bilinear":
            raise ValueError(f"JointResize(interpolation={self._interpolation!r}, antialias=True): only the bilinear "
                             "resize has an antialiased form")

    def __call__(self, images, boxes, classes):
        old_h, old_w = images.shape[-2:]
        new_h, new_w = self._size
        kw = {"align_corners": False} if self._interpolation in ("bilinear", "bicubic") else {}
        if self._antialias:
            kw["antialias"] = True
        images = F.interpolate(images, size=(new_h, new_w), mode=self._interpolation, **kw)
        boxes, classes = annotate(("resize", old_w, old_h, new_w, new_h), boxes, classes)
        return images, boxes, classes

    def _extend(self, plan, rng):
        if self._interpolation != "bilinear":
            raise ValueError(f"JointResize(interpolation={self._interpolation!r}) cannot be planned: the device pass is bilinear")
        if plan.photo is not None:
            raise ValueError("JointResize after a JointPhotometricDistortion cannot be planned: per-pixel colour work "
                             "does not commute with resampling (put the photometric step last)")
        if plan._resized:
            raise ValueError("JointResize after a JointResize cannot be planned: two resamplings are not one bilinear pass")
        if plan._flip_seen:
            raise ValueError("JointResize after a JointHorizontalFlip cannot be planned: the flip comes last")
        old_h, old_w = plan.size
        plan.size = (self._size[0], self._size[1])
        plan._resized = True
        plan.antialias = self._antialias
        plan.steps.append(("resize", old_w, old_h, self._size[1], self._size[0]))


class BaseCrop(JointTransform, ABC):
    @abstractmethod
    def _get_crop_param(self, image_h: int, image_w: int, rng) -> Tuple[int, int, int, int]:
        """(top, left, height, width) of the crop of an image_h x image_w frame."""

    def _checked(self, image_h, image_w, rng):
        top, left, crop_h, crop_w = self._get_crop_param(image_h, image_w, rng)
        if not (0 < crop_h <= image_h and 0 < crop_w <= image_w and 0 <= top <= image_h - crop_h
                and 0 <= left <= image_w - crop_w):
            raise ValueError(f"{type(self).__name__}: crop {crop_h}x{crop_w} at ({top}, {left}) leaves the "
                             f"{image_h}x{image_w} frame (padding crops are not supported)")
        return top, left, crop_h, crop_w

    def __call__(self, images, boxes, classes):
        image_h, image_w = images.shape[-2:]
        top, left, crop_h, crop_w = self._checked(image_h, image_w, _random)
        images = images[..., top:top + crop_h, left:left + crop_w]
        boxes, classes = annotate(("crop", left, top, crop_w, crop_h), boxes, classes)
        return images, boxes, classes

    def _extend(self, plan, rng):
        if plan._resized or plan._flip_seen:
            raise ValueError(f"{type(self).__name__} after a {'JointResize' if plan._resized else 'JointHorizontalFlip'} "
                             "cannot be planned: crops come first (a crop of resampled pixels is a second resampling)")
        image_h, image_w = plan.size
        top, left, crop_h, crop_w = self._checked(image_h, image_w, rng)
        plan.rect = (plan.rect[0] + top, plan.rect[1] + left, crop_h, crop_w)
        plan.size = (crop_h, crop_w)
        plan.steps.append(("crop", left, top, crop_w, crop_h))


class JointCenterCrop(BaseCrop):
    def __init__(self, size):
        self.th, self.tw = int(size[0]), int(size[1])

    def _get_crop_param(self, image_h, image_w, rng):
        return (image_h - self.th) // 2, (image_w - self.tw) // 2, self.th, self.tw


class JointRandomCrop(JointCenterCrop):
    def _get_crop_param(self, image_h, image_w, rng):
        if self.th > image_h or self.tw > image_w:
            return 0, 0, self.th, self.tw                      # refused by _checked
        return rng.randint(0, image_h - self.th), rng.randint(0, image_w - self.tw), self.th, self.tw


class RandomSizedCrop(BaseCrop):
    def __init__(self, min_scale, max_scale):
        assert max_scale <= 1.0, "Cannot crop more than the whole image!"
        self._min_scale, self._max_scale = min_scale, max_scale

    def _crop_size(self, image_h, image_w, rng):
        scale = rng.uniform(self._min_scale, self._max_scale)
        return int(image_h * scale), int(image_w * scale)

    def _get_crop_param(self, image_h, image_w, rng):
        crop_h, crop_w = self._crop_size(image_h, image_w, rng)
        return rng.randint(0, image_h - crop_h), rng.randint(0, image_w - crop_w), crop_h, crop_w


class CenterBiasedRandomSizedCrop(RandomSizedCrop):
    """The crop's origin follows a triangular distribution that peaks where the crop is centred."""

    def _get_crop_param(self, image_h, image_w, rng):
        crop_h, crop_w = self._crop_size(image_h, image_w, rng)
        max_i, max_j = image_h - crop_h + 1, image_w - crop_w + 1
        top = min(int(rng.triangular(0, max_i, max_i / 2)), max_i - 1)       # the closed upper end would leave the frame
        left = min(int(rng.triangular(0, max_j, max_j / 2)), max_j - 1)
        return top, left, crop_h, crop_w


class JointHorizontalFlip(JointTransform):
    def __init__(self, p: float = 0.5):
        self._p = p

    def __call__(self, images, boxes, classes):
        if _random.random() < self._p:
            images = images.flip(-1)
            boxes, classes = annotate(("flip", images.shape[-1]), boxes, classes)
        return images, boxes, classes

    def _extend(self, plan, rng):
        if plan._flip_seen:
            raise ValueError("JointHorizontalFlip after a JointHorizontalFlip cannot be planned: at most one flip")
        plan._flip_seen = True
        if rng.random() < self._p:
            plan.flip = True
            plan.steps.append(("flip", plan.size[1]))


class RandomSelect(JointTransform):
    """`transforms1` with probability p, else `transforms2`."""

    def __init__(self, transforms1, transforms2, p=0.5):
        self.transforms1, self.transforms2, self.p = transforms1, transforms2, p

    def __call__(self, *args, **kwargs):
        if _random.random() < self.p:
            return self.transforms1(*args, **kwargs)
        return self.transforms2(*args, **kwargs)

    def _extend(self, plan, rng):
        JointCompose([self.transforms1 if rng.random() < self.p else self.transforms2])._extend(plan, rng)


class SizeFilter(JointTransform):
    """Filter objects based on size (relative to image size)."""

    def __init__(self, min_size):
        self.min_size = min_size

    def __call__(self, images, boxes, classes):
        image_h, image_w = images.shape[-2:]
        boxes, classes = annotate(("size_filter", image_w, image_h, self.min_size), boxes, classes)
        return images, boxes, classes

    def _extend(self, plan, rng):
        plan.steps.append(("size_filter", plan.size[1], plan.size[0], self.min_size))


class JointPhotometricDistortion(JointTransform):
    """Brightness, contrast, saturation and hue jitter, drawn ONCE per clip and applied identically to all its frames
    (the standard colour augmentation of camera detectors; the reference has none).  The map is `photometric` above.

    Nine numbers are drawn, always, in this order -- so the generator ends in the same state whatever they decide:
        u_b, delta in [-brightness_delta, brightness_delta]      brightness is applied iff u_b < p
        u_c, alpha in contrast_range                             contrast likewise
        u_s, sat   in saturation_range                           saturation
        u_h, hue   in [-hue_delta, hue_delta] (turns)            hue
        u_f                                                      first = u_f < 0.5: contrast before the HSV stage
    A stage that is not applied takes its neutral value.  Boxes and classes pass through.

    `__call__` takes a float clip [L, 3, h, w] in 0..1 and does not normalise; with `pixel_mean` / `pixel_std` (three
    numbers each) the clip is a normalised one: it is de-normalised first and re-normalised after."""

    def __init__(self, brightness_delta=32 / 255, contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5),
                 hue_delta=18 / 360, p=0.5, pixel_mean=None, pixel_std=None):
        self._brightness_delta, self._hue_delta, self._p = float(brightness_delta), float(hue_delta), float(p)
        self._contrast_range = tuple(float(v) for v in contrast_range)
        self._saturation_range = tuple(float(v) for v in saturation_range)
        if not 0.0 <= self._brightness_delta <= 1.0:
            raise ValueError(f"brightness_delta {brightness_delta!r} is not in [0, 1] (the 0..1 scale)")
        if not 0.0 <= self._hue_delta <= 0.5:
            raise ValueError(f"hue_delta {hue_delta!r} is not in [0, 0.5] turns")
        for name, rng_ in (("contrast_range", self._contrast_range), ("saturation_range", self._saturation_range)):
            if len(rng_) != 2 or not 0.0 <= rng_[0] <= rng_[1] <= 4.0:
                raise ValueError(f"{name} {rng_!r} is not (low, high) with 0 <= low <= high <= 4")
        if not 0.0 <= self._p <= 1.0:
            raise ValueError(f"p {p!r} is not a probability")
        if (pixel_mean is None) != (pixel_std is None):
            raise ValueError("pixel_mean and pixel_std are given together or not at all")
        self._norm = None
        if pixel_mean is not None:
            mean, std = (torch.tensor([float(v) for v in t], dtype=torch.float32) for t in (pixel_mean, pixel_std))
            if mean.shape != (3,) or std.shape != (3,) or not bool((std > 0).all()):
                raise ValueError("pixel_mean / pixel_std are three numbers each, the deviations positive")
            self._norm = (mean.view(3, 1, 1), std.view(3, 1, 1))

    def _draw(self, rng):
        row = []
        for neutral, low, high in ((0.0, -self._brightness_delta, self._brightness_delta),
                                   (1.0, *self._contrast_range), (1.0, *self._saturation_range),
                                   (0.0, -self._hue_delta, self._hue_delta)):
            applied, value = rng.random() < self._p, rng.uniform(low, high)
            row.append(value if applied else neutral)
        row.append(1.0 if rng.random() < 0.5 else 0.0)
        return tuple(row)

    def __call__(self, images, boxes, classes):
        row = self._draw(_random)
        if self._norm is None:
            return photometric(images, row), boxes, classes
        mean, std = self._norm
        return (photometric(images * std + mean, row) - mean) / std, boxes, classes

    def _extend(self, plan, rng):
        if plan.photo is not None:
            raise ValueError("JointPhotometricDistortion after a JointPhotometricDistortion cannot be planned: a clip "
                             "has one photometric row")
        plan.photo = self._draw(rng)


def _inner(transform):
    """The transforms directly inside a JointCompose or a RandomSelect; nothing for any other step."""
    return list(getattr(transform, "transforms", ())) if isinstance(transform, JointCompose) else \
        [transform.transforms1, transform.transforms2] if isinstance(transform, RandomSelect) else []


def has_photometric(transform):
    """Whether a JointPhotometricDistortion stands anywhere in `transform` (inside JointCompose / RandomSelect too): then
    its plans may carry a row, and the device half takes the `photo` operand."""
    if isinstance(transform, JointPhotometricDistortion):
        return True
    return any(has_photometric(t) for t in _inner(transform))


def _resizes(transform):
    if isinstance(transform, JointResize):
        return [transform]
    return [r for t in _inner(transform) for r in _resizes(t)]


def uses_antialias(transform):
    """Whether the JointResize steps of `transform` (inside JointCompose / RandomSelect too) antialias: then the device
    half runs `fod_clip_crop_resize_aa`.  One tree makes one choice -- the device half reads it once, and a RandomSelect
    must not make it per sample: steps that disagree raise ValueError.  A tree without a JointResize does not."""
    flags = {r._antialias for r in _resizes(transform)}
    if len(flags) > 1:
        raise ValueError("the JointResize steps of one transform disagree on antialias: the device pass is chosen once "
                         "per transform, not per sample (give every JointResize the same flag)")
    return bool(flags) and flags.pop()
