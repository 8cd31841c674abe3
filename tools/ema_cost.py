#!/usr/bin/env python3
"""The captured training step of the headline model (bench.py's: B = 2, T = 6, 900 x 1600, bf16, all five past frames
live) with a weight EMA attached (future_od.optim.WeightEMA): a few replays, for a kernel trace that shows
`multi_ema_kernel` beside `multi_adamw_kernel`, and -- without the tracer -- the replay time with and without the EMA.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ema_cost.py --replays 5
        (a run of its own: the two kernels' average durations are read from DIR's kernel statistics)
    python tools/ema_cost.py --replays 20 --compare        (replay time of the step, EMA attached / detached, alternating)"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "future-object-detection_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--decay", type=float, default=0.9998)
    ap.add_argument("--size", type=int, nargs=4, default=[2, 6, 900, 1600], metavar=("B", "T", "H", "W"))
    ap.add_argument("--compare", action="store_true", help="also capture the step without the EMA and time both")
    a = ap.parse_args()

    import torch
    from future_od.datasets.synthetic import make_batch
    from future_od.graph import GraphedStep
    from future_od.models.st_detr import SpatioTemporalDETRArgs
    from future_od.optim import FusedAdamW, WeightEMA
    from runs._model import build_model
    if not torch.cuda.is_available():
        raise SystemExit("ema_cost: needs a GPU (a CPU run measures nothing)")
    dev = "cuda:0"
    B, T, H, W = a.size
    data = make_batch(B, T, H, W, seed=1234, device=dev)

    def build(with_ema):
        torch.manual_seed(0)
        args = SimpleNamespace(device=dev, distributed=False, compute_dtype="bf16", num_images=T - 1, attn_dtype="bf16")
        detr = SpatioTemporalDETRArgs(num_classes=8, num_queries=128, lr_backbone=1e-4, pretrained_backbone=False)
        model = build_model(args, detr)
        model.eval()                                 # bench.py's mode: eval-mode math with autograd on
        opt = FusedAdamW(model.parameters(), lr=detr.lr, weight_decay=detr.weight_decay, max_norm=detr.max_norm)
        ema = None
        if with_ema:
            ema = WeightEMA(model, decay=a.decay)
            opt.attach_ema(ema)
        step = GraphedStep(model, opt, warmup=2)
        for _ in range(a.warmup + 1):                # the first call captures
            step(data)
        torch.cuda.synchronize()
        return step, opt, ema

    steps = {"ema": build(True)}
    if a.compare:
        steps["plain"] = build(False)
    times = {k: [] for k in steps}
    for _ in range(a.replays):
        for k, (step, _, _) in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(data)
            torch.cuda.synchronize()
            times[k].append(1e3 * (time.perf_counter() - t0))
    _, opt, ema = steps["ema"]
    n = sum(t.numel() for _, t in ema.named_tensors())
    out = {"size": a.size, "replays": a.replays, "averaged_parameters": n, "bytes_moved_by_the_update": 12 * n,
           "num_updates": ema.num_updates, "optimizer_steps": opt._step_no,
           "replay_ms_median": {k: statistics.median(v) for k, v in times.items()},
           "replay_ms_min": {k: min(v) for k, v in times.items()}}
    assert out["num_updates"] == out["optimizer_steps"], out
    print(json.dumps(out))


if __name__ == "__main__":
    main()
