"""Shared by tests/test_antialias_cpu.py and tests/test_antialias_gpu.py: the antialiased resize of include/fod_ext.h
(fod_clip_crop_resize_aa) restated in a chosen precision, the normalisation, the plan row as the kernel clamps it, the
cases and their recorded limits.  Nothing here imports the project: it is what the class and the kernel are held
against.

The kernel's tiling is 16 x 64 outputs a workgroup: the cases marked "tiles" span at least two tiles in both directions
with the seams inside; 128 x 512 -> 32 x 128 does so at the accepted ratio limit of 4."""
import torch

MEAN, STD = torch.tensor([0.485, 0.456, 0.406]), torch.tensor([0.229, 0.224, 0.225])
MAX_RATIO = 4                                # frame / output per axis the entry point must accept


def taps(n_in, n_out, dtype):
    """The definition, per axis: -> the [n_out, n_in] matrix of normalised weights in `dtype` (zero outside [lo, hi)).
    Scalars are formed in `dtype` too: scale = n_in / n_out is ROUNDED to it, as torch rounds it for a float32 clip."""
    one = torch.ones((), dtype=dtype)
    scale = torch.tensor(n_in, dtype=dtype) / torch.tensor(n_out, dtype=dtype)
    sup = torch.maximum(scale, one)
    m = torch.zeros(n_out, n_in, dtype=dtype)
    for i in range(n_out):
        c = scale * (i + 0.5)
        lo = max(0, int(c - sup + 0.5))
        hi = min(n_in, int(c + sup + 0.5))
        j = torch.arange(lo, hi, dtype=dtype)
        w = (1 - ((j - c + 0.5) / sup).abs()).clamp(min=0)
        m[i, lo:hi] = w / w.sum()
    return m


def sample(crop_u8, size, dtype):
    """[..., h, w] uint8 -> [..., H, W] in `dtype` on the 0..255 scale: the horizontal pass, then the vertical one."""
    h, w = crop_u8.shape[-2:]
    my, mx = taps(h, size[0], dtype), taps(w, size[1], dtype)
    return my @ (crop_u8.to(dtype) @ mx.t())


def normalise(p):
    """0..1 planes [..., C, h, w] -> normalised units, in p's precision (C = 1 takes the first mean / std)."""
    c = p.shape[-3]
    return (p - MEAN[:c].to(p.dtype).view(c, 1, 1)) / STD[:c].to(p.dtype).view(c, 1, 1)


def restated(crop_u8, size, dtype):
    """A cropped clip [..., C, h, w] -> what fod_clip_crop_resize_aa defines for it, every step in `dtype`."""
    return normalise(sample(crop_u8, size, dtype) / 255)


def clamped(plan, h0, w0):
    """(top, left, height, width, flip) as the kernel reads it: the extent is clamped into the frame, then the origin."""
    top, left, h, w, flip = plan
    h, w = min(max(h, 1), h0), min(max(w, 1), w0)
    return min(max(top, 0), h0 - h), min(max(left, 0), w0 - w), h, w, int(flip != 0)


def source(case):
    """The case's raw clip [B, L, C, H0, W0] uint8.  "noise": random bytes; "white": 255 everywhere; "pixel": black with
    one 255 pixel in every plane.  A padded case lives in storage with 37 spare bytes after every frame."""
    B, L, C, H0, W0 = case["B"], case["L"], case["C"], case["H0"], case["W0"]
    g = torch.Generator().manual_seed(1000 * H0 + W0)
    if case["kind"] == "noise":
        u8 = torch.randint(0, 256, (B, L, C, H0, W0), generator=g, dtype=torch.uint8)
    elif case["kind"] == "white":
        u8 = torch.full((B, L, C, H0, W0), 255, dtype=torch.uint8)
    else:
        u8 = torch.zeros(B, L, C, H0, W0, dtype=torch.uint8)
        u8[..., H0 // 2, W0 // 2] = 255
    if not case.get("padded"):
        return u8
    n = C * H0 * W0
    store = torch.randint(0, 256, (B, L, n + 37), generator=g, dtype=torch.uint8)
    store[:, :, :n] = u8.view(B, L, n)
    return store                              # the test views store[:, :, :n] as [B, L, C, H0, W0] (on its device)


def view(store, case):
    if not case.get("padded"):
        return store
    n = case["C"] * case["H0"] * case["W0"]
    return store[:, :, :n].view(case["B"], case["L"], case["C"], case["H0"], case["W0"])


def expected(case, u8, dtype, fn=None):
    """-> [B, L, C, H, W]: `fn(crop, size)` (default: the restatement in `dtype`) per sample on its clamped rectangle,
    columns mirrored where the plan flips."""
    fn = fn or (lambda crop, size: restated(crop, size, dtype))
    out = []
    for b, plan in enumerate(case["plans"]):
        top, left, h, w, flip = clamped(plan, case["H0"], case["W0"])
        e = fn(u8[b, :, :, top:top + h, left:left + w], case["size"])
        out.append(e.flip(-1) if flip else e)
    return torch.stack(out)


def _case(name, H0, W0, size, plans, C=3, L=1, kind="noise", **kw):
    return dict(name=name, B=len(plans), L=L, C=C, H0=H0, W0=W0, size=size, plans=plans, kind=kind, **kw)


CASES = [
    _case("37x53 to 12x20, ratios 3.1 / 2.65", 37, 53, (12, 20), [(0, 0, 37, 53, 0)]),
    _case("45x80 to 28x50, ratio 1.6, flip, W % 4 = 2", 45, 80, (28, 50), [(0, 0, 45, 80, 1)]),
    _case("50x90 to 24x44, ratio about 2", 50, 90, (24, 44), [(0, 0, 50, 90, 0)]),
    _case("white frame", 50, 90, (24, 44), [(0, 0, 50, 90, 0)], kind="white"),
    _case("single bright pixel", 50, 90, (24, 44), [(0, 0, 50, 90, 0), (3, 2, 45, 85, 1)], kind="pixel"),
    _case("30x50 unchanged at the four frame borders", 45, 80, (30, 50),
          [(0, 13, 30, 50, 0), (15, 20, 30, 50, 1), (7, 0, 30, 50, 0), (9, 30, 30, 50, 1)], unchanged=True),
    _case("11x13 to 22x26, up, one plane", 11, 13, (22, 26), [(0, 0, 11, 13, 0)], C=1),
    _case("20x60 to 32x24, one axis up and one down", 40, 70, (32, 24), [(10, 5, 20, 60, 0), (20, 10, 20, 60, 1)]),
    _case("output 1x1 at the ratio limit", 3, 4, (1, 1), [(0, 0, 3, 4, 0), (1, 1, 2, 3, 1)]),
    _case("W = 7", 20, 25, (9, 7), [(0, 0, 20, 25, 0), (2, 3, 17, 21, 1)]),
    _case("W = 61, one plane", 70, 150, (33, 61), [(0, 0, 70, 150, 1), (1, 9, 66, 130, 0)], C=1),
    _case("tiles: 90x330 to 40x150, two clips of two padded frames, one rectangle leaves the frame", 96, 340, (40, 150),
          [(3, 5, 90, 330, 0), (20, 100, 90, 330, 1)], L=2, padded=True),
    _case("tiles: 128x512 to 32x128, the ratio limit", 128, 512, (32, 128), [(0, 0, 128, 512, 0), (0, 0, 128, 512, 1)]),
]
# one step past the accepted limit, per axis: (H0, W0, (H, W))
PAST_LIMIT = [(65, 256, (16, 64)), (64, 257, (16, 64))]

# The limits.  For each case: the largest distance, on normalised outputs, between torch's float32 CPU evaluation
# (F.interpolate(antialias=True) on the float32 crop, / 255, normalised) and the float64 restatement above, times three,
# rounded up to two digits.  tests/test_antialias_cpu.py measures each again and fails if a figure here is below three
# times the distance, or more than six times it.  The kernel is held to these on every output element.
# Where a ratio is no float32 number (1.6, 2.04, ...) the distance is the rounding of `scale` carried into the weights,
# about 1e-5; where it is one (4, 1, 0.5) only the sums' own roundings are left, a few 1e-7.
LIMITS = {
    "37x53 to 12x20, ratios 3.1 / 2.65": 4.3e-06,
    "45x80 to 28x50, ratio 1.6, flip, W % 4 = 2": 2.2e-05,
    "50x90 to 24x44, ratio about 2": 1.7e-05,
    "white frame": 2.7e-06,
    "single bright pixel": 2.6e-06,
    "30x50 unchanged at the four frame borders": 7.6e-07,
    "11x13 to 22x26, up, one plane": 5.2e-07,
    "20x60 to 32x24, one axis up and one down": 1.8e-06,
    "output 1x1 at the ratio limit": 7.1e-07,
    "W = 7": 2.5e-06,
    "W = 61, one plane": 3.0e-05,
    "tiles: 90x330 to 40x150, two clips of two padded frames, one rectangle leaves the frame": 5.7e-05,
    "tiles: 128x512 to 32x128, the ratio limit": 1.4e-06,
}

# The same rule with a photometric row between the sample and the normalisation (photometric_cases.restated): on the
# PHOTO_CASE rectangles, row by row.
PHOTO_CASE = _case("photo rows: 50x90 to 24x44 and 45x70 to 24x44", 50, 90, (24, 44), [(0, 0, 50, 90, 0), (5, 20, 45, 70, 1)],
                   L=2)
PHOTO_LIMITS = {
    "brightness": 1.8e-05,
    "darker": 1.7e-05,
    "contrast": 2.4e-05,
    "contrast down": 9.4e-06,
    "saturation": 2.3e-05,
    "desaturation": 1.5e-05,
    "hue": 1.7e-05,
    "hue back": 2.4e-05,
    "all, contrast after": 2.9e-05,
    "all, contrast first": 1.1e-05,
}

# DeviceJointTransform end to end: raw frames, the output size, the clips of a batch, the transform's seed.  The limit is
# three times the per-sample CPU transform's own distance to the float64 restatement of its plans, as above.
E2E = dict(raw=(90, 160), size=(40, 72), B=3, L=2, seed=21)
E2E_LIMIT = 4.4e-05
