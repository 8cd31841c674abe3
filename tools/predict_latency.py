#!/usr/bin/env python3
"""Replay time of label-free inference (future_od.graph.GraphedPredict) next to the evaluation pass (GraphedForward) on
ONE resident batch at the headline extent (B = 2, T = 6, 900 x 1600, bf16, all five past frames live; bench.py's
model): the two graphs are replayed in turn, each replay between device synchronisations, and the medians are reported.
predict replays a strict subset of forward's launches plus one node (fod_detect_select), so its time must not exceed
forward's.

    python tools/predict_latency.py --out profiles/predict_latency.json
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/predict_latency.py --predict-only --replays 5
        (a run of its own: the duration of detect_select_kernel is read from DIR's kernel statistics)
    ... --predict-only --replays 5 --nms 0.5 [--top-k 300]
        (duplicate suppression as one more node of the graph: detect_nms_kernel stands beside detect_select_kernel in
        the same statistics; tools/measure_nms.py measures the two on rows whose suppressed share is set)"""
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
    ap.add_argument("--replays", type=int, default=30, help="timed replays of each graph (alternating)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--top-k", type=int, default=100)
    ap.add_argument("--size", type=int, nargs=4, default=[2, 6, 900, 1600], metavar=("B", "T", "H", "W"))
    ap.add_argument("--nms", type=float, default=None, metavar="THR",
                    help="predict(nms=THR): one fod_detect_nms launch behind the selection, inside the graph")
    ap.add_argument("--nms-class-agnostic", action="store_true")
    ap.add_argument("--predict-only", action="store_true", help="replay GraphedPredict alone (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from future_od.datasets.synthetic import make_batch
    from future_od.graph import GraphedForward, GraphedPredict
    from future_od.models.st_detr import SpatioTemporalDETRArgs
    from runs._model import build_model
    if not torch.cuda.is_available():
        raise SystemExit("predict_latency: needs a GPU (a CPU run measures nothing)")
    dev = "cuda:0"
    B, T, H, W = a.size
    torch.manual_seed(0)
    args = SimpleNamespace(device=dev, distributed=False, compute_dtype="bf16", num_images=T - 1, attn_dtype="bf16")
    model = build_model(args, SpatioTemporalDETRArgs(num_classes=8, num_queries=128, lr_backbone=1e-4,
                                                     pretrained_backbone=False))
    model.eval()
    data = make_batch(B, T, H, W, seed=1234, device=dev)
    passes = {"predict": GraphedPredict(model, top_k=a.top_k, nms=a.nms, nms_class_agnostic=a.nms_class_agnostic)}
    if not a.predict_only:
        passes["forward"] = GraphedForward(model)
    for _ in range(a.warmup + 1):                    # the first call captures
        for fn in passes.values():
            fn(data)
    torch.cuda.synchronize()
    times = {k: [] for k in passes}
    for _ in range(a.replays):
        for k, fn in passes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(data)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    det = passes["predict"](data)
    torch.cuda.synchronize()
    line = {"what": "graph replay, host clock around replay + device synchronise, graphs alternating on one resident batch",
            "extent": {"B": B, "T": T, "H": H, "W": W, "dtype": "bf16", "num_images": T - 1, "top_k": a.top_k},
            "replays_each": a.replays, "device": torch.cuda.get_device_name(0),
            "detections": [int(c) for c in det["count"].tolist()]}
    if a.nms is not None:
        line["nms"] = {"iou_threshold": a.nms, "class_agnostic": a.nms_class_agnostic}
    for k, ts in times.items():
        line[f"{k}_ms_median"] = round(statistics.median(ts), 4)
        line[f"{k}_ms_min"] = round(min(ts), 4)
        line[f"{k}_ms_max"] = round(max(ts), 4)
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(line, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
