"""What duplicate suppression costs (profiles/detect_nms_cost.txt): fod_detect_nms beside fod_detect_select at
B = 2, M = 300 queries, C = 9 classes, K = 100 / 300 / 1024 rows, on clustered boxes of which about a third is suppressed
at iou_threshold 0.5, and once more on the same rows with nothing suppressed (iou_threshold 1: an IoU never exceeds it).

    python tools/measure_nms.py [--out FILE]                   device events around captured graphs
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/measure_nms.py --trace
    python tools/measure_nms.py --summarise DIR [--out FILE]   kernel durations of that trace, launch by launch

The head is synthetic, so the share of suppressed rows is set and not left to an untrained model: the queries fall into
groups that share a box (up to 1 % jitter), K (query, class) pairs carry high logits and everything else a low one, so
the selection returns exactly those K rows; two of them suppress each other iff they share group and class.  The
suppressed share of every configuration is counted from the kernel's own output, which is compared with the CPU form
(detect.detect_nms on host tensors) byte for byte first.
Events: a block of launches of each kernel is captured into a hipGraph and the graphs are replayed in alternation, so
the figure is a launch inside a graph, gaps between nodes included.  Trace: every configuration launches each kernel
eagerly --launches times, in a fixed order; the summary cuts the trace's rows for the two kernels into those runs.
The bytes a launch has to move, and the time they alone would take at the 8 TB/s of HBM3E, stand beside each figure: both
kernels are far from that bound -- they are one workgroup per sample and latency-bound.  A measurement needs the GPU."""
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

B, M, C, H, W = 2, 300, 9, 900, 1600
KS = (100, 300, 1024)
MODES = (("a third suppressed", 0.5), ("nothing suppressed", 1.0))
BLOCK, ROUNDS = 200, 12
HBM_BYTES_PER_US = 8e6                                   # 8 TB/s
KERNELS = ("detect_select_kernel", "detect_nms_kernel")


def synthetic_head(K, seed=0):
    """logits f32 [B,M,C], boxes f32 [B,M,4] cxcywh in (0,1): 0.128 K groups (so that K rows fall on about 1.15 K
    (group, class) combinations, of which about two thirds get hit) and K chosen (query, class) pairs per sample."""
    g = torch.Generator().manual_seed(seed + K)
    G = max(1, round(0.128 * K))
    centre = 0.15 + 0.7 * torch.rand(B, G, 2, generator=g)
    size = 0.05 + 0.15 * torch.rand(B, G, 2, generator=g)
    group = torch.randint(0, G, (B, M), generator=g)
    bi = torch.arange(B)[:, None]
    boxes = torch.cat([centre[bi, group] + 0.01 * size[bi, group] * (torch.rand(B, M, 2, generator=g) - 0.5),
                       size[bi, group] * (1 + 0.01 * (torch.rand(B, M, 2, generator=g) - 0.5))], dim=2)
    logits = torch.full((B, M * C), -8.0)
    for b in range(B):
        chosen = torch.randperm(M * C, generator=g)[:K]
        logits[b, chosen] = torch.linspace(4.0, 1.0, K)
    return logits.view(B, M, C).contiguous(), boxes.contiguous()


def select_bytes(K):
    return B * (M * C * 4 + M * 16 + K * 28 + 4)


def nms_bytes(K):
    return B * (K * 28 + 4 + K * 32 + 4)                  # every row read once, every row (and its source) written once


def configurations(dev):
    from future_od.native import detect
    for K in KS:
        logits, boxes = (t.to(dev) for t in synthetic_head(K))
        sel = detect.detect_select(logits, boxes, H, W, K)
        out = tuple(torch.empty_like(t) for t in sel + (sel[1],))
        for mode, thr in MODES:
            got = detect.detect_nms(*sel, thr, False, out=out)
            want = detect.detect_nms(*(t.cpu() for t in sel), thr, False)
            assert all(g.cpu().numpy().tobytes() == w.numpy().tobytes() for g, w in zip(got, want)), "the CPU form differs"
            kept = got[4].tolist()
            assert sel[4].tolist() == [K] * B
            yield dict(K=K, mode=mode, thr=thr, kept=kept,
                       select=lambda l=logits, b=boxes, K=K, s=sel: detect.detect_select(l, b, H, W, K, out=s),
                       nms=lambda s=sel, t=thr, o=out: detect.detect_nms(*s, t, False, out=o))


def _line(name, ts, nbytes):
    med = statistics.median(ts)
    return (f"{name:58s} median {med:7.1f} us   min {min(ts):7.1f}   max {max(ts):7.1f}   {nbytes:7d} B: "
            f"{nbytes / HBM_BYTES_PER_US:6.4f} us at 8 TB/s")


def _header(how):
    return [f"command: python tools/measure_nms.py {how}",
            f"B = {B} samples, M = {M} queries, C = {C} classes, {H} x {W} frame; class-aware; fod_detect_select ranks "
            f"M x C = {M * C} candidates (4096 sorted keys) for every K", ""]


def events(args):
    dev = torch.device("cuda:0")

    def captured(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(BLOCK):
                fn()
        graph.replay()
        torch.cuda.synchronize()
        return graph

    def block(graph):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / BLOCK          # us per launch

    graphs = {}
    for c in configurations(dev):
        share = 1 - sum(c["kept"]) / (B * c["K"])
        if c["mode"] == MODES[0][0]:
            graphs[f"fod_detect_select, K = {c['K']}"] = (captured(c["select"]), select_bytes(c["K"]))
        graphs[f"fod_detect_nms, K = {c['K']}, {c['mode']} ({100 * share:.0f} %: {c['kept']} kept)"] = \
            (captured(c["nms"]), nms_bytes(c["K"]))
    times = {name: [] for name in graphs}
    for _ in range(ROUNDS):                               # alternating: drift hits all alike
        for name, (graph, _) in graphs.items():
            times[name].append(block(graph))
    lines = _header(f"  ({torch.cuda.get_device_name(0)})")
    lines.insert(2, f"device events around a captured graph of {BLOCK} launches, {ROUNDS} alternating replays per kernel; us per "
                    f"launch, the gap between two nodes of a graph included")
    lines += [_line(name, ts, graphs[name][1]) for name, ts in times.items()]
    return lines


def trace(args):
    """Eager launches in the order summarise() expects; the suppressed shares go to the sidecar file the summary reads."""
    dev = torch.device("cuda:0")
    notes = []
    for c in configurations(dev):
        torch.cuda.synchronize()
        for fn in (c["select"], c["nms"]):
            for _ in range(args.launches):
                fn()
            torch.cuda.synchronize()
        notes.append(f"{c['K']}\t{c['mode']}\t{1 - sum(c['kept']) / (B * c['K']):.4f}\t{c['kept']}")
    if args.notes:
        with open(args.notes, "w") as f:
            f.write("\n".join(notes) + "\n")
    print("\n".join(notes))


def summarise(args):
    (path,) = glob.glob(os.path.join(args.summarise, "**", "*kernel_trace.csv"), recursive=True)
    rows = sorted((r for r in csv.DictReader(open(path)) if any(k in r["Kernel_Name"] for k in KERNELS)),
                  key=lambda r: int(r["Start_Timestamp"]))
    us = {k: [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if k in r["Kernel_Name"]]
          for k in KERNELS}
    n = args.launches
    # per K one select that produces the rows, per configuration one nms that is compared with the CPU form, then n of each
    notes = [ln.rstrip("\n").split("\t") for ln in open(args.notes)] if args.notes and os.path.isfile(args.notes) else None
    lines = _header("--trace, under rocprofv3 --kernel-trace; then --summarise")
    lines.insert(2, f"kernel durations (end - start of the dispatch) of {n} eager launches per kernel and configuration, one trace")
    k = 0
    sel_at = nms_at = 0
    for K in KS:
        sel_at += 1                                       # the launch that produced the rows
        for mi, (mode, _) in enumerate(MODES):
            nms_at += 1                                   # the launch that was compared with the CPU form
            sel = us[KERNELS[0]][sel_at:sel_at + n]
            nms = us[KERNELS[1]][nms_at:nms_at + n]
            sel_at += n
            nms_at += n
            share = f" ({100 * float(notes[k][2]):.0f} %: {notes[k][3]} kept)" if notes else ""
            lines.append(_line(f"fod_detect_select, K = {K} (before the next line)", sel, select_bytes(K)))
            lines.append(_line(f"fod_detect_nms, K = {K}, {mode}{share}", nms, nms_bytes(K)))
            k += 1
    assert sel_at == len(us[KERNELS[0]]) and nms_at == len(us[KERNELS[1]]), (sel_at, nms_at, len(us[KERNELS[0]]), len(us[KERNELS[1]]))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true", help="eager launches only, to be run under rocprofv3 --kernel-trace")
    ap.add_argument("--launches", type=int, default=20, help="eager launches per kernel and configuration (--trace)")
    ap.add_argument("--notes", default=None, help="sidecar file: --trace writes the suppressed shares, --summarise reads them")
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
