"""What the streaming AP costs (profiles/ap_hist_cost.txt): fod_ap_hist_accum beside the fod_detect_od_map launch that
feeds it, fod_ap_hist_finalize, and the wall time of aggregate_mean_average_precision on 500 concatenated batches of the
same rows.  B = 2, M = 300 queries, C = 9 classes, K = 300 rows, per_class = 50, T = 10 (the configuration of
tools/measure_detect_od_map.py, whose synthetic head and annotations are reused).

    python tools/measure_ap_hist.py [--out FILE]                         device events and the wall time of the aggregation
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/measure_ap_hist.py --trace
    python tools/measure_ap_hist.py --summarise DIR [--out FILE --append]    kernel durations of that trace

Before anything is timed the kernels' state and outputs are compared with the CPU form (integers, pr and pr_score byte
for byte).  The bytes a launch has to move, and the time they alone would take at the 8 TB/s of HBM3E, stand beside each
figure.  The accumulation reads every flag, one score and T positives per filled slot and issues one 4-byte integer atomic
per (slot, size flag) and per true positive of it: a launch of a few thousand threads, bound by its launch and the
atomics' latency, not by bytes.  The finalisation reads the whole state once from memory (hist_tp once per row, hist_seen
by the T rows that share it, the second pass from the L2) and writes a few KB: its cost is the state's size, whatever
the number of batches.  A measurement needs the GPU."""
import argparse
import csv
import glob
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "future-object-detection_amd")
sys.path[:0] = [ROOT, PKG, os.path.join(ROOT, "tools")]

import torch  # noqa: E402

import measure_detect_od_map as MD  # noqa: E402

B, M, C, N, H, W = MD.B, MD.M, MD.C, MD.N, MD.H, MD.W
K, PER_CLASS, T = 300, 50, 10
C1, P = C + 1, B * PER_CLASS
NB = 0x3F81
BLOCK, ROUNDS, BATCHES = 200, 12, 500
HBM_BYTES_PER_US = 8e6
KERNELS = ("detect_od_map_kernel", "ap_hist_accum_kernel", "ap_hist_finalize_kernel")
STATE_BYTES = (T * C1 * 4 * NB * 4, C1 * 4 * NB * 4 + C1 * 4 * 8)


def setup(dev):
    from future_od.native import detect
    logits, boxes, anno, classes, active = (t.to(dev) for t in MD.synthetic())
    sel = detect.detect_select(logits, boxes, H, W, K)
    od = detect.detect_od_map(*sel, anno, classes, active, (H, W), C, PER_CLASS, T=T)
    state = detect.ap_hist_state(T, C1, dev)
    detect.ap_hist_accum(od, state)
    host = detect.ap_hist_state(T, C1, "cpu")
    detect.ap_hist_accum(tuple(t.cpu() for t in od), host)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(state, host)), "the CPU form's histograms differ"
    got, want = detect.ap_hist_finalize(state), detect.ap_hist_finalize(host)
    assert all(got[k].cpu().numpy().tobytes() == want[k].numpy().tobytes() for k in (2, 3, 4)), "the CPU form's curve differs"
    filled, adds = int(od[2][:, 0].sum()), int(state[1].sum()) + int(state[0].sum())
    accum_bytes = C1 * 4 * P + filled * (4 + T) + C1 * 4 * 8 + adds * 4
    final_bytes = sum(STATE_BYTES) + T * C1 * 4 * (8 + 8 + 101 * 12 + 16)
    run = dict(detect=lambda: detect.detect_od_map(*sel, anno, classes, active, (H, W), C, PER_CLASS, T=T, out=od),
               accum=lambda: detect.ap_hist_accum(od, state), finalize=lambda: detect.ap_hist_finalize(state))
    names = dict(detect=f"fod_detect_od_map, K = {K} ({filled} of {C1 * P} slots filled)",
                 accum=f"fod_ap_hist_accum ({filled} filled slots, {adds} integer atomics)",
                 finalize=f"fod_ap_hist_finalize ({T * C1 * 4} rows of {NB} bins; state {STATE_BYTES[0] / 1e6:.1f} MB + "
                          f"{STATE_BYTES[1] / 1e6:.1f} MB)")
    nbytes = dict(detect=MD.detect_bytes(K), accum=accum_bytes, finalize=final_bytes)
    return od, state, run, names, nbytes


def _line(name, ts, nbytes):
    med = statistics.median(ts)
    return (f"{name:92s} median {med:8.1f} us   min {min(ts):8.1f}   max {max(ts):8.1f}   {nbytes:9d} B: "
            f"{nbytes / HBM_BYTES_PER_US:7.4f} us at 8 TB/s")


def _header(how):
    return [f"command: python tools/measure_ap_hist.py {how}",
            f"B = {B} samples, M = {M} queries, C = {C} classes (+ the generic class), K = {K} rows, per_class = {PER_CLASS}, "
            f"T = {T}: {P} slots per class and batch", ""]


def events(args):
    from future_od.utils.od_map import aggregate_mean_average_precision
    dev = torch.device("cuda:0")
    od, state, run, names, nbytes = setup(dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(BLOCK):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / BLOCK

    lines = _header(f"  ({torch.cuda.get_device_name(0)})")
    lines.insert(2, f"device events around {BLOCK} eager calls, {ROUNDS} rounds; us per call, launch cost included")
    for k in ("detect", "accum", "finalize"):
        timed(run[k])
        lines.append(_line(names[k], [timed(run[k]) for _ in range(ROUNDS)], nbytes[k]))
    # what the streaming state replaces: the sorted aggregation over every batch's tensors, on the same device
    cat = (od[0].repeat(1, 1, BATCHES), od[1].repeat(1, 1, BATCHES), od[2].repeat(1, 1, BATCHES),
           od[3][:, :, None].repeat(1, 1, BATCHES))
    kept = sum(t.numel() * t.element_size() for t in cat)
    wall = []
    with open(os.devnull, "w") as null:
        for _ in range(5):
            torch.cuda.synchronize()
            t0, out = time.perf_counter(), sys.stdout
            sys.stdout = null                                # (it prints the annotation counts)
            try:
                aggregate_mean_average_precision(*cat, dev)
            finally:
                sys.stdout = out
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e6)
    lines += ["", f"aggregate_mean_average_precision on {BATCHES} concatenated batches ({P * BATCHES} slots per class, {kept / 1e6:.1f} MB "
                  f"kept on the device), wall time of the call, 5 calls (the first includes its warm-up):",
              "    " + "  ".join(f"{w / 1e3:.2f} ms" for w in wall),
              f"the streaming state: {sum(STATE_BYTES) / 1e6:.1f} MB whatever the number of batches"]
    return lines


def trace(args):
    dev = torch.device("cuda:0")
    od, state, run, names, nbytes = setup(dev)
    torch.cuda.synchronize()
    notes = []
    for k, kernel in zip(("detect", "accum", "finalize"), KERNELS):
        for _ in range(args.launches):
            run[k]()
        torch.cuda.synchronize()
        notes.append(f"{kernel}\t{nbytes[k]}\t{names[k]}")
    if args.notes:
        with open(args.notes, "w") as f:
            f.write("\n".join(notes) + "\n")
    print("\n".join(notes))


def summarise(args):
    (path,) = glob.glob(os.path.join(args.summarise, "**", "*kernel_trace.csv"), recursive=True)
    word = lambda r: next((k for k in KERNELS if k in r["Kernel_Name"]), None)
    rows = sorted((r for r in csv.DictReader(open(path)) if word(r)), key=lambda r: int(r["Start_Timestamp"]))
    us = {k: [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if word(r) == k] for k in KERNELS}
    n = args.launches
    lines = _header("--trace, under rocprofv3 --kernel-trace --stats; then --summarise")
    lines.insert(2, f"kernel durations (end - start of the dispatch) of the last {n} eager launches of each kernel, one trace")
    for kernel, nbytes, name in (ln.rstrip("\n").split("\t") for ln in open(args.notes)):
        assert len(us[kernel]) >= n, (kernel, len(us[kernel]))
        lines.append(_line(name, us[kernel][-n:], int(nbytes)))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    ap.add_argument("--trace", action="store_true", help="eager launches only, to be run under rocprofv3 --kernel-trace")
    ap.add_argument("--launches", type=int, default=20, help="eager launches per kernel (--trace)")
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
        with open(args.out, "a" if args.append else "w") as f:
            f.write(("\n" if args.append else "") + text)


if __name__ == "__main__":
    main()
