"""What the tracker's launch costs (profiles/track_update_cost.txt): fod_track_update beside fod_detect_select and
fod_detect_nms in ONE kernel trace, at B = 2, K = 100 / 300 / 1024 rows and S = 256 / 1024 slots, from three states:

  two thirds matched   min(2K/3, S) tracks, each under a row of its own on a grid of disjoint boxes: every claim is the
                       row's first choice (the scalar path of the walk); the other rows are born while slots are free
  all births           an empty state: nothing to claim, every row is born while slots are free
  first choice taken   min(K, S) tracks in a row, a quarter of a box apart; row 0 sits on track 0, row j >= 1 nearest to
                       track j - 1, which row j - 1 has taken: every row but the first recomputes its arg-max over the
                       unclaimed slots (the slow path of the walk)

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/measure_track.py --trace --notes FILE
    python tools/measure_track.py --summarise DIR --notes FILE [--out FILE]    kernel durations, launch by launch

The launch changes the state it reads, so every measured launch starts from a copy of the same state (the copies are
other kernels: the summary does not count them).  The selection and the suppression run on the synthetic head of
tools/measure_nms.py; the tracker's rows are synthetic as well, so that the three states are what they are called: the
numbers of matched and born rows of every configuration are counted from the kernel's own output, which is compared
with the CPU form (detect.track_update on host tensors) byte for byte first.
The bytes a launch moves at most, and the time they alone would take at the 8 TB/s of HBM3E, stand beside each figure.
A measurement needs the GPU."""
import argparse
import csv
import glob
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "future-object-detection_amd")
sys.path[:0] = [ROOT, PKG, os.path.join(ROOT, "tools")]

import torch  # noqa: E402

import measure_nms as MN  # noqa: E402

B = MN.B
KS, SS = (100, 300, 1024), (256, 1024)
STATES = ("two thirds matched", "all births", "first choice taken")
PARAMS = dict(iou_threshold=0.3, birth_score=0.0, max_misses=3, class_agnostic=False, motion=True)
KERNELS = ("detect_select_kernel", "detect_nms_kernel", "track_update_kernel")
HBM_BYTES_PER_US = 8e6


def track_bytes(K, S):
    """At most: 24 B read and 12 B written per row, 52 B read and 52 B written per slot, count and next_id."""
    return B * (K * 36 + S * 104 + 12)


def empty_state(S):
    meta = torch.zeros(B, S, 4, dtype=torch.int32)
    meta[:, :, :2] = -1
    return [torch.zeros(B, S, 4), torch.zeros(B, S, 4), meta, torch.zeros(B, S), torch.zeros(B, dtype=torch.int32)]


def rows_and_state(K, S, which):
    """-> (scores, labels, boxes, count), state: host tensors."""
    scores = torch.linspace(0.99, 0.05, K)[None].repeat(B, 1).contiguous()
    labels = torch.zeros(B, K, dtype=torch.int32)
    count = torch.full((B,), K, dtype=torch.int32)
    state = empty_state(S)
    k = torch.arange(K, dtype=torch.float32)
    if which == "first choice taken":
        x = torch.where(k > 0, (k - 0.6) * 10.0, torch.zeros(()))
        boxes = torch.stack([x, torch.zeros(K), x + 40.0, torch.full((K,), 40.0)], dim=1)
        T = min(K, S)
        t = torch.arange(T, dtype=torch.float32) * 10.0
        tracks = torch.stack([t, torch.zeros(T), t + 40.0, torch.full((T,), 40.0)], dim=1)
    else:
        x, y = (k % 32) * 50.0, (k // 32) * 50.0            # a grid of disjoint 40 x 40 boxes
        boxes = torch.stack([x, y, x + 40.0, y + 40.0], dim=1)
        T = 0 if which == "all births" else min(2 * K // 3, S)
        tracks = boxes[torch.arange(T) * 3 // 2] + 1.0       # under two rows of every three, one pixel off
    state[0][:, :T] = tracks
    state[2][:, :T] = torch.stack([torch.arange(T), torch.zeros(T), torch.ones(T), torch.zeros(T)], dim=1).to(torch.int32)
    state[3][:, :T] = 0.5
    state[4][:] = T
    return (scores, labels, boxes[None].repeat(B, 1, 1).contiguous(), count), state


def configurations(dev):
    from future_od.native import detect
    for K in KS:
        logits, hboxes = (t.to(dev) for t in MN.synthetic_head(K))
        sel = detect.detect_select(logits, hboxes, MN.H, MN.W, K)
        nms_out = tuple(torch.empty_like(t) for t in sel + (sel[1],))
        for S in SS:
            for which in STATES:
                rows, pristine = rows_and_state(K, S, which)
                want_state = [t.clone() for t in pristine]
                want = detect.track_update(*rows, want_state, **PARAMS)
                rows, pristine = tuple(t.to(dev) for t in rows), [t.to(dev) for t in pristine]
                state = [t.clone() for t in pristine]
                out = tuple(torch.empty_like(rows[1]) for _ in range(3))
                got = detect.track_update(*rows, state, **PARAMS, out=out)
                assert all(g.cpu().numpy().tobytes() == w.numpy().tobytes() for g, w in zip(tuple(state) + got, tuple(want_state) + want)), \
                    "the CPU form differs"
                matched, born = int((got[1] > 1).sum()), int((got[1] == 1).sum())
                if which == "first choice taken":         # row j took track j: never its nearest one, j - 1
                    T = min(K, S)
                    assert got[2][0, :T].tolist() == list(range(T)) and matched == B * T

                def track(rows=rows, state=state, pristine=pristine, out=out):
                    for s, p in zip(state, pristine):
                        s.copy_(p)
                    detect.track_update(*rows, state, **PARAMS, out=out)
                yield dict(K=K, S=S, which=which, matched=matched, born=born, track=track,
                           select=lambda l=logits, b=hboxes, K=K, s=sel: detect.detect_select(l, b, MN.H, MN.W, K, out=s),
                           nms=lambda s=sel, o=nms_out: detect.detect_nms(*s, 0.5, False, out=o))


def _line(name, ts, nbytes):
    med = statistics.median(ts)
    return (f"{name:78s} median {med:7.1f} us   min {min(ts):7.1f}   max {max(ts):7.1f}   {nbytes:7d} B: "
            f"{nbytes / HBM_BYTES_PER_US:6.4f} us at 8 TB/s")


def trace(args):
    """Eager launches in the order summarise() expects; what was matched and born goes to the sidecar file."""
    dev = torch.device("cuda:0")
    notes = []
    for c in configurations(dev):
        torch.cuda.synchronize()
        for fn in (c["select"], c["nms"], c["track"]):
            for _ in range(args.launches):
                fn()
            torch.cuda.synchronize()
        notes.append(f"{c['K']}\t{c['S']}\t{c['which']}\t{c['matched']}\t{c['born']}")
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
    notes = [ln.rstrip("\n").split("\t") for ln in open(args.notes)] if args.notes and os.path.isfile(args.notes) else None
    lines = ["command: python tools/measure_track.py --trace, under rocprofv3 --kernel-trace; then --summarise",
             f"B = {B} samples; iou_threshold {PARAMS['iou_threshold']}, birth_score {PARAMS['birth_score']}, class-aware, "
             f"motion on; fod_detect_select and fod_detect_nms (iou_threshold 0.5) as in tools/measure_nms.py",
             f"kernel durations (end - start of the dispatch) of {n} eager launches per kernel and configuration, one trace", ""]
    at = {k: 0 for k in KERNELS}
    i = 0
    for K in KS:
        at[KERNELS[0]] += 1                                 # the launch that produced the rows of the suppression
        for S in SS:
            for which in STATES:
                at[KERNELS[2]] += 1                         # the launch that was compared with the CPU form
                cut = {k: us[k][at[k]:at[k] + n] for k in KERNELS}
                for k in KERNELS:
                    at[k] += n
                what = f" ({notes[i][3]} matched, {notes[i][4]} born)" if notes else ""
                if S == SS[0] and which == STATES[0]:
                    lines.append(_line(f"fod_detect_select, K = {K}", cut[KERNELS[0]], MN.select_bytes(K)))
                    lines.append(_line(f"fod_detect_nms, K = {K}, a third suppressed", cut[KERNELS[1]], MN.nms_bytes(K)))
                lines.append(_line(f"fod_track_update, K = {K}, S = {S}, {which}{what}", cut[KERNELS[2]], track_bytes(K, S)))
                i += 1
    assert all(at[k] == len(us[k]) for k in KERNELS), (at, {k: len(v) for k, v in us.items()})
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true", help="eager launches, to be run under rocprofv3 --kernel-trace")
    ap.add_argument("--launches", type=int, default=20, help="eager launches per kernel and configuration")
    ap.add_argument("--notes", default=None, help="sidecar file: --trace writes what was matched and born, --summarise reads it")
    ap.add_argument("--summarise", default=None, metavar="DIR", help="read the kernel trace below DIR (no GPU needed)")
    args = ap.parse_args()
    if args.summarise:
        text = "\n".join(summarise(args)) + "\n"
        print(text, end="")
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(text)
        return
    assert torch.cuda.is_available() and args.trace, "a measurement needs the GPU: run --trace under rocprofv3 --kernel-trace"
    trace(args)


if __name__ == "__main__":
    main()
