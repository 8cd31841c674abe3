"""fod_clip_crop_resize at the two stage extents of the shipped schedule, next to the uint8 stem ingest of the same clip.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/measure_augment.py
    python tools/measure_augment.py --summarize OUT/<host>/<pid>_kernel_trace.csv

The first form only launches (one 2 x 6 x 3 x 900 x 1600 uint8 noise clip; outputs (448, 800) and (896, 1600), crop
scale 0.5 and 1.0, WARM + REPS launches each, then the stem's layout kernel on the raw clip); the second reads the
trace (dispatch order = launch order) and prints, per configuration, the bytes the kernel needs -- output
4*B*L*3*H*W plus source B*L*3*height*width, from the shapes -- over the median kernel time."""
import os
import sys

B, L, H0, W0 = 2, 6, 900, 1600
WARM, REPS = 3, 20
CONFIGS = [(size, scale) for size in ((448, 800), (896, 1600)) for scale in (0.5, 1.0)]


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
    for size, scale in CONFIGS:
        h, w = int(H0 * scale), int(W0 * scale)
        plans = torch.tensor([((H0 - h) // 2, (W0 - w) // 2, h, w, 0), (H0 - h, W0 - w, h, w, 1)], dtype=torch.int32,
                             device=dev)
        for _ in range(WARM + REPS):
            ops.clip_crop_resize(u8, plans, size, mean, std)
        torch.cuda.synchronize()
    for _ in range(WARM + REPS):
        ops.clip_to_stem_layout(u8, torch.bfloat16, mean, std)
    torch.cuda.synchronize()
    print("launched", len(CONFIGS) * (WARM + REPS), "crop/resize and", WARM + REPS, "stem layout kernels")


def summarize(path):
    import csv
    import statistics
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3
    crop = [r for r in rows if "clip_crop_resize_kernel" in r["Kernel_Name"]]
    stem = [r for r in rows if "stem_layout_kernel" in r["Kernel_Name"]]
    assert len(crop) == len(CONFIGS) * (WARM + REPS) and len(stem) == WARM + REPS, (len(crop), len(stem))
    print(f"clip {B} x {L} x 3 x {H0} x {W0} uint8; median of {REPS} launches after {WARM}; achievable HBM ~6.3 TB/s")
    print("kernel                       output       source       bytes needed  median us   min us   TB/s")
    for i, (size, scale) in enumerate(CONFIGS):
        h, w = int(H0 * scale), int(W0 * scale)
        nbytes = 4 * B * L * 3 * size[0] * size[1] + B * L * 3 * h * w
        t = [us(r) for r in crop[i * (WARM + REPS) + WARM:(i + 1) * (WARM + REPS)]]
        med = statistics.median(t)
        print(f"clip_crop_resize_kernel      {size[0]:>4}x{size[1]:<7} {h:>4}x{w:<7} {nbytes:>12}  {med:9.1f}  {min(t):7.1f}  "
              f"{nbytes / med * 1e-6:5.2f}")
    hp, wp = max(2 * ((H0 - 1) // 2 + 1) + 5, H0 + 3), max(2 * ((W0 - 1) // 2 + 1) + 6, W0 + 3 + ((W0 + 3) & 1))
    nbytes = B * L * 3 * H0 * W0 + B * L * hp * wp * 4 * 2            # raw planes in, haloed 4-channel bf16 frames out
    t = [us(r) for r in stem[WARM:]]
    med = statistics.median(t)
    print(f"stem_layout_kernel<bf16,u8>  {hp:>4}x{wp}x4    {H0:>4}x{W0:<7} {nbytes:>12}  {med:9.1f}  {min(t):7.1f}  "
          f"{nbytes / med * 1e-6:5.2f}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        launch()
