"""What the AP bookkeeping over detection rows costs (profiles/detect_od_map_cost.txt): fod_detect_od_map beside
fod_od_map on the same predictions, B = 2, M = 300 queries, C = 9 classes, N = 40 annotation slots per sample,
K = 100 / 300 / 1024 rows, per_class = 50, T = 10.

    python tools/measure_detect_od_map.py [--out FILE]                   device events around captured graphs
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/measure_detect_od_map.py --trace
    python tools/measure_detect_od_map.py --summarise DIR [--out FILE]   kernel durations of that trace, launch by launch

The head is random (logits randn * 2, boxes that are jittered copies of the annotations or random), the rows are what
fod_detect_select returns for every K, and the kernel's output is compared with the CPU form (detect.detect_od_map on host
tensors) byte for byte before anything is timed.
Events: per configuration a block of calls is captured into a hipGraph; replays of it alternate with the same block
launched eagerly, so there are two figures per call: inside a graph, gaps between nodes included, and eager, launch
cost included.  One graph is alive at a time, and a replay into poisoned outputs is compared with the reference first.
Trace: every configuration launches each kernel eagerly --launches times, in a fixed order; the summary cuts the trace's
rows into those runs.
The bytes a launch has to move (every input once, every output once), and the time they alone would take at the 8 TB/s
of HBM3E, stand beside each figure: both kernels are far from that bound -- a serial walk over at most 50 candidates
per workgroup, latency-bound.  A measurement needs the GPU."""
import argparse
import csv
import glob
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "future-object-detection_amd")
sys.path[:0] = [ROOT, PKG]

import torch  # noqa: E402

B, M, C, N, H, W = 2, 300, 9, 40, 900, 1600
KS = (100, 300, 1024)
PER_CLASS, T = 50, 10
BLOCK, ROUNDS = 200, 12
HBM_BYTES_PER_US = 8e6                                   # 8 TB/s
# (od_map_zero_kernel also holds the first name: the trace's rows are matched on the whole word)
KERNELS = ("od_map_kernel", "detect_od_map_kernel")


def synthetic(seed=0):
    """logits f32 [B,M,C], boxes f32 [B,M,4] cxcywh in (0,1), annotations: boxes f32 [B,N,4] xyxy px, classes, active."""
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand(B, N, 2, generator=g) * torch.tensor([W * 0.8, H * 0.8])
    wh = 20 + torch.rand(B, N, 2, generator=g) * torch.tensor([W * 0.18, H * 0.18])
    anno = torch.cat([xy, xy + wh], dim=2)
    classes = torch.randint(0, C, (B, N), generator=g)
    active = (torch.rand(B, N, generator=g) < 0.8).long()
    src = torch.randint(0, N, (B, M), generator=g)
    px = anno[torch.arange(B)[:, None], src] + 6 * (torch.rand(B, M, 4, generator=g) - 0.5)
    rnd = torch.rand(B, M, 2, generator=g) * torch.tensor([W * 0.8, H * 0.8])
    rnd = torch.cat([rnd, rnd + 20 + torch.rand(B, M, 2, generator=g) * 200], dim=2)
    px = torch.where(torch.rand(B, M, 1, generator=g) < 0.7, px, rnd)
    scale = torch.tensor([W, H, W, H], dtype=torch.float32)
    boxes = torch.cat([(px[..., :2] + px[..., 2:]) / 2, px[..., 2:] - px[..., :2]], dim=2) / scale
    logits = torch.randn(B, M, C, generator=g) * 2
    return logits.contiguous(), boxes.contiguous(), anno.contiguous(), classes, active


def od_map_bytes():
    P = min(50, M)
    return B * (M * (C + 1) * 4 + M * 16 + N * 32) + _out_bytes(P)


def detect_bytes(K):
    return B * (K * 28 + 4 + N * 32) + _out_bytes(min(PER_CLASS, K))


def _out_bytes(P):
    C1 = C + 1
    return T * C1 * B * P * 5 + C1 * 4 * B * P + C1 * 4 * 8


def configurations(dev):
    from future_od.native import detect
    logits, boxes, anno, classes, active = (t.to(dev) for t in synthetic())
    scores, boxes_px = detect.post_proc(logits, boxes, H, W)
    dense = detect.od_map(scores, boxes_px, anno, classes, active, (H, W))
    yield dict(name="fod_od_map (dense scores, 2 launches)", bytes=od_map_bytes(), kernel=KERNELS[0], out=None,
               fn=lambda: detect.od_map(scores, boxes_px, anno, classes, active, (H, W)))
    for K in KS:
        sel = detect.detect_select(logits, boxes, H, W, K)
        assert sel[4].tolist() == [K] * B
        out = detect.detect_od_map(*sel, anno, classes, active, (H, W), C, PER_CLASS, T=T)
        want = detect.detect_od_map(*(t.cpu() for t in sel), anno.cpu(), classes.cpu(), active.cpu(), (H, W), C, PER_CLASS, T=T)
        assert all(g.cpu().numpy().tobytes() == w.numpy().tobytes() for g, w in zip(out, want)), "the CPU form differs"
        filled = int(out[2][:, 0].sum())
        tp = int((out[1][0] & out[2][:, 0]).sum())
        yield dict(name=f"fod_detect_od_map, K = {K} ({filled} of {(C + 1) * B * min(PER_CLASS, K)} slots filled, {tp} positive "
                        f"at IoU 0.5; dense: {int(dense[1][0].sum())})", bytes=detect_bytes(K), kernel=KERNELS[1], out=out,
                   fn=lambda s=sel, o=out: detect.detect_od_map(*s, anno, classes, active, (H, W), C, PER_CLASS, T=T, out=o))


def _line(name, ts, nbytes):
    med = statistics.median(ts)
    return (f"{name:104s} median {med:7.1f} us   min {min(ts):7.1f}   max {max(ts):7.1f}   {nbytes:7d} B: "
            f"{nbytes / HBM_BYTES_PER_US:6.4f} us at 8 TB/s")


def _header(how):
    return [f"command: python tools/measure_detect_od_map.py {how}",
            f"B = {B} samples, M = {M} queries, C = {C} classes (+ the generic class), N = {N} annotation slots, {H} x {W} "
            f"frame, per_class = {PER_CLASS}, T = {T}; fod_od_map ranks the {M} dense scores of every class itself", ""]


def events(args):
    dev = torch.device("cuda:0")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / BLOCK          # us per call

    lines = _header(f"  ({torch.cuda.get_device_name(0)})")
    lines.insert(2, f"device events around {BLOCK} calls: a captured graph of them and the same calls launched eagerly, {ROUNDS} "
                    f"alternating rounds per configuration; us per call")
    for c in configurations(dev):
        fn = c["fn"]
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(BLOCK):
                fn()
        if c["out"] is not None:                          # the replay does the work: poisoned outputs come back right
            want = [t.clone() for t in c["out"]]
            c["out"][0].fill_(3.0)
            c["out"][1].fill_(True)
            graph.replay()
            assert all(torch.equal(a, b) for a, b in zip(c["out"], want)), "a replay left other outputs"
        graph.replay()
        in_graph, eager = [], []
        for _ in range(ROUNDS):
            in_graph.append(timed(graph.replay))
            eager.append(timed(lambda: [fn() for _ in range(BLOCK)]))
        lines.append(_line(c["name"] + "  in a graph", in_graph, c["bytes"]))
        lines.append(_line(" " * len(c["name"]) + "  eager", eager, c["bytes"]))
        del graph
    return lines


def trace(args):
    """Eager launches in the order summarise() expects; the configurations' names go to the sidecar file."""
    dev = torch.device("cuda:0")
    notes = []
    for c in configurations(dev):
        torch.cuda.synchronize()
        for _ in range(args.launches):
            c["fn"]()
        torch.cuda.synchronize()
        notes.append(f"{c['kernel']}\t{c['bytes']}\t{c['name']}")
    if args.notes:
        with open(args.notes, "w") as f:
            f.write("\n".join(notes) + "\n")
    print("\n".join(notes))


def summarise(args):
    (path,) = glob.glob(os.path.join(args.summarise, "**", "*kernel_trace.csv"), recursive=True)

    def word(r):
        name = r["Kernel_Name"]
        return KERNELS[1] if KERNELS[1] in name else KERNELS[0] if KERNELS[0] in name else None
    rows = sorted((r for r in csv.DictReader(open(path)) if word(r) in KERNELS), key=lambda r: int(r["Start_Timestamp"]))
    us = {k: [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if word(r) == k] for k in KERNELS}
    n = args.launches
    notes = [ln.rstrip("\n").split("\t") for ln in open(args.notes)]
    lines = _header("--trace, under rocprofv3 --kernel-trace; then --summarise")
    lines.insert(2, f"kernel durations (end - start of the dispatch) of {n} eager launches per configuration, one trace; "
                    f"fod_od_map: od_map_kernel alone, its zeroing launch not counted")
    at = {k: 0 for k in KERNELS}
    for kernel, nbytes, name in notes:
        at[kernel] += 1                                   # the launch whose result was looked at (od_map: the dense reference)
        lines.append(_line(name, us[kernel][at[kernel]:at[kernel] + n], int(nbytes)))
        at[kernel] += n
    assert all(at[k] == len(us[k]) for k in KERNELS), (at, {k: len(v) for k, v in us.items()})
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true", help="eager launches only, to be run under rocprofv3 --kernel-trace")
    ap.add_argument("--launches", type=int, default=20, help="eager launches per configuration (--trace)")
    ap.add_argument("--notes", default=None, help="sidecar file: --trace writes the configurations, --summarise reads them")
    ap.add_argument("--summarise", default=None, metavar="DIR", help="read the kernel trace below DIR (no GPU needed)")
    args = ap.parse_args()
    if args.summarise:
        lines = summarise(args)
    else:
        assert torch.cuda.is_available(), "a measurement needs the GPU"
        if args.trace:
            return trace(args)
        lines = events(args)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
