#!/usr/bin/env python3
"""The device matcher's launch alone (fod_lap_solve_batch_dev), timed with HIP events: warm-up, then the median of single
timed launches, at Lv = 6 decoder levels and B = 2 samples (12 problems, one wavefront each).

    python tools/lap_cost.py [--launches 30] [--parent-lib PARENT/libfod_hip.so] [--out FILE]

  * M = 128, ld = 256 (the headline step's launch, costs staged by the host's decision).  With --parent-lib (a library built
    from the parent commit) the two libraries alternate launch by launch in one process, the parent's twice per round, so
    the spread it shows against itself stands next to the difference.
  * M = 300, ld = 256 (Conditional DETR's default query count; every workgroup stages its own n x 300 costs when
    n * 300 <= FOD_LAP_STAGE_FLOATS): n = 8, 40, the largest n that still stages, the first that does not, 256."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "future-object-detection_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

LV, B = 6, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=30, help="timed launches per configuration (at least 20)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libfod_hip.so of another commit to alternate with at M = 128")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    a = ap.parse_args()
    assert a.launches >= 20

    import numpy as np
    import torch
    from future_od.native import lib as L
    if not torch.cuda.is_available():
        raise SystemExit("lap_cost: needs a GPU (a CPU run measures nothing)")
    dev = "cuda:0"
    libs = {"this": L.LIB}
    if a.parent_lib:
        other = C.CDLL(os.path.abspath(a.parent_lib))
        L._typed(other, "fod_lap_solve_batch_dev")
        libs["parent"] = other
    stream = torch.cuda.current_stream(dev).cuda_stream
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    def problem(M, ld, n):
        rng = np.random.default_rng(M * 7919 + n * 31 + ld)
        cost = torch.from_numpy(rng.standard_normal((LV, B, M, ld)).astype(np.float32) * 3).to(dev)
        off = torch.tensor([0, n, 2 * n], dtype=torch.int32, device=dev)
        match = torch.empty((LV, B, M), dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        return cost, off, match, status

    def launch(lib, prob):
        cost, off, match, status = prob
        _, _, M, ld = cost.shape
        rc = lib.fod_lap_solve_batch_dev(cost.data_ptr(), LV * B, B, M, ld, off.data_ptr(), match.data_ptr(),
                                         status.data_ptr(), stream)
        if rc:
            raise SystemExit(f"lap_cost: fod_lap_solve_batch_dev({M}, {ld}) returned {rc}: {L.last_error()}")

    def timed(lib, prob):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch(lib, prob)
        e1.record()
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1)                            # us

    def row(label, us):
        q = statistics.quantiles(us, n=4)
        return f"  {label:<34s} median {statistics.median(us):9.1f} us   min {min(us):9.1f}   quartiles {q[0]:9.1f} .. {q[2]:9.1f}"

    say(f"fod_lap_solve_batch_dev alone, Lv = {LV}, B = {B}: {a.warmup} warm-up + {a.launches} launches timed one by one "
        f"(HIP events), {torch.cuda.get_device_name(0)}")
    say()
    say("M = 128, ld = 256, n = 40 per sample (the headline step's launch form)")
    prob = problem(128, 256, 40)
    order = [("this", "this commit")] if len(libs) == 1 else \
        [("parent", "parent library, first slot"), ("this", "this commit"), ("parent", "parent library, second slot")]
    times = [[] for _ in order]
    for r in range(a.warmup + a.launches):
        for k in range(len(order)):
            slot = (k + r) % len(order)                            # rotate who goes first
            t = timed(libs[order[slot][0]], prob)
            if r >= a.warmup:
                times[slot].append(t)
    assert int(prob[3].item()) == 0
    for (_, label), us in zip(order, times):
        say(row(label, us))
    if len(order) == 3:
        med = [statistics.median(us) for us in times]
        say(f"  this commit - parent library: {med[1] - 0.5 * (med[0] + med[2]):+.1f} us;  parent library against itself "
            f"(second slot - first): {med[2] - med[0]:+.1f} us")
    say()
    stage = L.LAP_STAGE_FLOATS
    last = stage // 300
    say(f"M = 300, ld = 256 (staged in LDS when n * 300 <= {stage}, i.e. n <= {last}; otherwise read from global memory)")
    for n in (8, 40, last, last + 1, 256):
        prob = problem(300, 256, n)
        for _ in range(a.warmup):
            launch(L.LIB, prob)
        us = [timed(L.LIB, prob) for _ in range(a.launches)]
        assert int(prob[3].item()) == 0
        say(row(f"n = {n:3d} ({'LDS' if n * 300 <= stage else 'global'})", us))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
