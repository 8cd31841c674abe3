#!/usr/bin/env python
"""Record what the reference's own draw_boxes paints, as data: tests/golden/draw_boxes_ref.npz.

    python tests/golden/make_render_golden.py <reference checkout>

The reference's future_od/utils/visualization.py is imported as it is; `wandb` and `torchvision`, which it imports at
its top and which draw_boxes does not use, are empty stand-in modules -- nothing else is stubbed.  The drawable geometry
cases of tests/render_cases.py with at most 16 boxes are run (the many-box cases are noise that does not compress, and
say nothing about the map that the others do not): no NaN coordinate (the reference raises on one), the first sample of
a case, and the label filter applied beforehand the way the reference's `visualize` applies its own (rows whose label is out of
range are dropped, the colours are COLOURS[label]).  The background is a small repeating pattern, one per frame size,
so that the file stays a few KB.  Stored: the inputs (image, boxes, colours, thickness) and the float outputs."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import render_cases as RC  # noqa: E402


def load_reference(checkout):
    for name in ("wandb", "torchvision"):
        sys.modules.setdefault(name, types.ModuleType(name))
    path = os.path.join(checkout, "future_od", "utils", "visualization.py")
    spec = importlib.util.spec_from_file_location("reference_visualization", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def pattern(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([((y * 3 + x + c) % 8).astype(np.float32) / np.float32(8) for c in range(3)])


def main(checkout):
    ref = load_reference(checkout)
    images, outs, names, rows = {}, {}, [], []
    for case in RC.geometry_cases():
        boxes, labels = case["boxes"][0], case["labels"][0]
        if np.isnan(boxes).any() or len(boxes) > 16:
            continue
        keep = (labels >= 0) & (labels < len(ref.COLOURS))
        h, w = case["video"].shape[-2:]
        size = f"{h}x{w}"
        images.setdefault(size, pattern(h, w))
        colours = ref.COLOURS[torch.from_numpy(labels[keep]).long()]
        image = torch.from_numpy(images[size].copy())
        painted = ref.draw_boxes(image, torch.from_numpy(boxes[keep]), colours, case["thickness"])
        n = int(keep.sum())
        pad_boxes, pad_colours = np.zeros((16, 4), np.float32), np.zeros((16, 3), np.float32)
        pad_boxes[:n], pad_colours[:n] = boxes[keep], colours.numpy()
        rows.append((h, w, case["thickness"], n, len(outs.setdefault(size, [])), pad_boxes, pad_colours))
        outs[size].append(painted.numpy())
        names.append(case["name"])
    # few, large arrays: a zip member costs more than a small case's data
    np.savez_compressed(os.path.join(HERE, "draw_boxes_ref.npz"), names=np.array(names),
                        meta=np.array([r[:5] for r in rows], dtype=np.int32),      # h, w, thickness, boxes, slot in out_<h>x<w>
                        boxes=np.stack([r[5] for r in rows]), colours=np.stack([r[6] for r in rows]),
                        **{f"image_{k}": v for k, v in images.items()}, **{f"out_{k}": np.stack(v) for k, v in outs.items()})
    print(f"{len(names)} cases -> draw_boxes_ref.npz")


if __name__ == "__main__":
    main(sys.argv[1])
