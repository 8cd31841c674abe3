"""Shared by tests/test_photometric_cpu.py and tests/test_photometric_gpu.py: the photometric map of include/fod_ext.h
(fod_clip_crop_resize_photo) restated in a chosen precision, the row as the kernel sanitises it, and the pixels the
tests use.  Nothing here imports the project: it is what the class and the kernel are held against."""
import numpy as np
import torch

MEAN, STD = torch.tensor([0.485, 0.456, 0.406]), torch.tensor([0.229, 0.224, 0.225])
NEUTRAL = (0.0, 1.0, 1.0, 0.0, 0.0)

# (name, row): every stage alone, all together in both contrast orders
ROWS = {
    "brightness": (0.11, 1.0, 1.0, 0.0, 0.0),
    "darker": (-0.09, 1.0, 1.0, 0.0, 1.0),
    "contrast": (0.0, 1.37, 1.0, 0.0, 1.0),
    "contrast down": (0.0, 0.55, 1.0, 0.0, 0.0),
    "saturation": (0.0, 1.0, 1.45, 0.0, 0.0),
    "desaturation": (0.0, 1.0, 0.5, 0.0, 1.0),
    "hue": (0.0, 1.0, 1.0, 0.04, 0.0),
    "hue back": (0.0, 1.0, 1.0, -0.05, 1.0),
    "all, contrast after": (0.08, 1.3, 1.4, 0.03, 0.0),
    "all, contrast first": (-0.06, 0.7, 0.6, -0.045, 1.0),
}


def normalise(p):
    """0..1 planes [..., 3, h, w] -> normalised units, in p's precision."""
    return (p - MEAN.to(p.dtype).view(3, 1, 1)) / STD.to(p.dtype).view(3, 1, 1)


def sanitised(row):
    """(delta, alpha, sat, hue, first) as the header says the kernel reads it, float32 arithmetic written out."""
    f32 = np.float32
    with np.errstate(all="ignore"):
        delta, alpha, sat, hue, first = (f32(v) for v in row)
        delta = f32(0) if not np.isfinite(delta) else min(max(delta, f32(-1)), f32(1))
        alpha = f32(1) if not np.isfinite(alpha) else min(max(alpha, f32(0)), f32(4))
        sat = f32(1) if not np.isfinite(sat) else min(max(sat, f32(0)), f32(4))
        hue = f32(0) if not np.isfinite(hue) else f32(hue - np.floor(hue))
    return float(delta), float(alpha), float(sat), float(hue), 0.0 if first == 0 else 1.0


def restated(p, row, dtype):
    """Steps 1-5 of the definition on planes [..., 3, h, w] in 0..1, every step in `dtype`; the row is sanitised first
    (its numbers are float32 values, as the kernel holds them)."""
    delta, alpha, sat, hue, first = sanitised(row)
    p = p.to(dtype)
    if (delta, alpha, sat, hue) == NEUTRAL[:4]:
        return p
    zero, one = torch.zeros((), dtype=dtype), torch.ones((), dtype=dtype)
    p = p + delta
    if first:
        p = p * alpha
    if sat != 1 or hue != 0:
        p = torch.minimum(torch.maximum(p, zero), one)
        r, g, b = p[..., 0, :, :], p[..., 1, :, :], p[..., 2, :, :]
        v, m = p.amax(dim=-3), p.amin(dim=-3)
        c = v - m
        flat = c <= 0
        c1, v1 = torch.where(flat, one, c), torch.where(flat, one, v)
        s = torch.where(flat, zero, c / v1)
        red = (g - b) / c1
        red = torch.where(red < 0, red + 6, red)                       # fmod(., 6) of a number in [-1, 1], non-negative
        h6 = torch.where(flat, zero, torch.where(v == r, red, torch.where(v == g, (b - r) / c1 + 2, (r - g) / c1 + 4)))
        h = h6 / 6
        s = torch.minimum(s * sat, one)
        h = h + hue
        h = h - torch.floor(h)
        out = []
        for n in (5, 3, 1):
            k = torch.fmod(n + 6 * h, 6)
            out.append(v - v * s * torch.maximum(zero, torch.minimum(torch.minimum(k, 4 - k), one)))
        p = torch.stack(out, dim=-3)
    if not first:
        p = p * alpha
    return torch.minimum(torch.maximum(p, zero), one)


# grey, black, white, the primaries and their complements, ties r == g, g == b, r == b (as maximum and as minimum),
# near-grey (a tiny chroma: the hue is badly conditioned, the output is not) and dark saturated pixels
STRUCTURED_U8 = [
    (128, 128, 128), (0, 0, 0), (255, 255, 255), (37, 37, 37),
    (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255),
    (200, 200, 40), (40, 200, 200), (200, 40, 200), (40, 40, 200), (200, 40, 40), (40, 200, 40),
    (129, 128, 128), (128, 129, 128), (128, 128, 129), (3, 0, 0), (0, 2, 1), (1, 0, 250),
]


def structured_frames(L, h, w, seed, patch=8):
    """uint8 noise frames [L, 3, h, w] whose top rows hold `patch` x `patch` blocks of the structured pixels."""
    g = torch.Generator().manual_seed(seed)
    u8 = torch.randint(0, 256, (L, 3, h, w), generator=g, dtype=torch.uint8)
    per_row = max(w // patch, 1)
    for i, rgb in enumerate(STRUCTURED_U8):
        y, x = (i // per_row) * patch, (i % per_row) * patch
        if y + patch <= h:
            u8[:, :, y:y + patch, x:x + patch] = torch.tensor(rgb, dtype=torch.uint8).view(1, 3, 1, 1)
    return u8
