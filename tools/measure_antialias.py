"""fod_clip_crop_resize_aa at the two stage extents of the shipped schedule -- without and with a photometric row --
next to fod_clip_crop_resize on the same clips in the same trace (the recipe of tools/measure_photometric.py).

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/measure_antialias.py
    python tools/measure_antialias.py --summarize OUT/<host>/<pid>_kernel_trace.csv

The first form only launches (one 2 x 6 x 3 x 900 x 1600 uint8 noise clip; outputs (448, 800) and (896, 1600), crop
scale 0.5 and 1.0; per configuration WARM + REPS launches of the antialiased kernel without rows, then with active
rows, then of the parent kernel); the second reads the trace (dispatch order = launch order) and prints, per
configuration, the three median kernel times, the ratio to the parent, and the bytes the pass needs -- output
4*B*L*3*H*W plus source B*L*3*height*width, the same for all three -- over the antialiased kernel's median."""
import os
import sys

B, L, H0, W0 = 2, 6, 900, 1600
WARM, REPS = 3, 20
CONFIGS = [(size, scale) for size in ((448, 800), (896, 1600)) for scale in (0.5, 1.0)]
ACTIVE = [(0.08, 1.3, 1.4, 0.03, 0.0), (-0.06, 0.7, 0.6, -0.045, 1.0)]      # every stage, both contrast orders


def launch():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "future-object-detection_amd")]
    import torch
    from future_od.native import ops
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    u8 = torch.randint(0, 256, (B, L, 3, H0, W0), generator=g, dtype=torch.uint8).to(dev)
    mean = torch.tensor([0.485, 0.456, 0.406], device=dev)
    std = torch.tensor([0.229, 0.224, 0.225], device=dev)
    active = torch.tensor(ACTIVE, dtype=torch.float32, device=dev)
    for size, scale in CONFIGS:
        h, w = int(H0 * scale), int(W0 * scale)
        plans = torch.tensor([((H0 - h) // 2, (W0 - w) // 2, h, w, 0), (H0 - h, W0 - w, h, w, 1)], dtype=torch.int32,
                             device=dev)
        for rows in (None, active):
            for _ in range(WARM + REPS):
                ops.clip_crop_resize_aa(u8, plans, size, mean, std, rows)
            torch.cuda.synchronize()
        for _ in range(WARM + REPS):
            ops.clip_crop_resize(u8, plans, size, mean, std)
        torch.cuda.synchronize()
    print("launched", 2 * len(CONFIGS) * (WARM + REPS), "antialiased and", len(CONFIGS) * (WARM + REPS), "parent kernels")


def summarize(path):
    import csv
    import statistics
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3
    aa = [r for r in rows if "clip_crop_resize_aa_kernel" in r["Kernel_Name"]]
    parent = [r for r in rows if "clip_crop_resize_kernel" in r["Kernel_Name"]]
    n = WARM + REPS
    assert len(aa) == 2 * len(CONFIGS) * n and len(parent) == len(CONFIGS) * n, (len(aa), len(parent))
    med = lambda rs: statistics.median(us(r) for r in rs[WARM:])
    print(f"clip {B} x {L} x 3 x {H0} x {W0} uint8; median of {REPS} launches after {WARM}; kernel times in us")
    print("output       source       bytes needed  antialiased  with photo row   parent  antialiased / parent  antialiased TB/s")
    for i, (size, scale) in enumerate(CONFIGS):
        h, w = int(H0 * scale), int(W0 * scale)
        nbytes = 4 * B * L * 3 * size[0] * size[1] + B * L * 3 * h * w
        plain, photo = med(aa[2 * i * n:(2 * i + 1) * n]), med(aa[(2 * i + 1) * n:(2 * i + 2) * n])
        par = med(parent[i * n:(i + 1) * n])
        print(f"{size[0]:>4}x{size[1]:<7} {h:>4}x{w:<7} {nbytes:>12}  {plain:11.1f}  {photo:14.1f}  {par:7.1f}  "
              f"{plain / par:20.2f}  {nbytes / plain * 1e-6:16.2f}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        launch()
