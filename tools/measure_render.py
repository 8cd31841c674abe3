"""What a visualisation costs (profiles/render_boxes_cost.txt): fod_render_boxes at 2 x 6 x 3 x 900 x 1600 f32 with 300
boxes per sample, with and without tile culling, beside what the reference does instead on the same box -- `video.cpu()`
of that clip.

    python tools/measure_render.py [--out FILE]

The product library stages only the boxes whose bars can reach a block's tile (csrc/render.hip, RB_CULL 1).  The other
form is the same file compiled with -DRB_CULL=0 into tools/bin/librender_nocull.so (built here when it is missing) and
called through ctypes with the prototype the binding reads from the header.  A block of launches of each form is
captured into a hipGraph (the launching thread's Python per call would otherwise be part of what is timed), and the
two graphs are replayed in alternation between device events, so the spread between blocks of ONE form is seen beside
the difference between the two; their pictures are compared byte for byte first.  A measurement needs the GPU: without
one this fails."""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "future-object-detection_amd")
sys.path[:0] = [ROOT, PKG]

import torch  # noqa: E402

NOCULL = os.path.join(ROOT, "tools", "bin", "librender_nocull.so")
B, L, H, W, N, BLOCK, ROUNDS = 2, 6, 900, 1600, 300, 50, 12


def build_nocull():
    if not os.path.isfile(NOCULL):
        os.makedirs(os.path.dirname(NOCULL), exist_ok=True)
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-Wno-comment", "-shared",
                               "-DRB_CULL=0", os.path.join(PKG, "csrc", "render.hip"), os.path.join(PKG, "csrc", "api.cpp"),
                               "-o", NOCULL])
    return NOCULL


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    from future_od.native import abi, ops
    from future_od.utils import visualization as V
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    video = torch.randn(B, L, 3, H, W, generator=g).to(dev)
    wh = torch.rand(B, N, 2, generator=g) * torch.tensor([W * 0.3, H * 0.3]) + 8.0
    xy = torch.rand(B, N, 2, generator=g) * (torch.tensor([float(W), float(H)]) - wh)
    boxes = torch.cat([xy, xy + wh], dim=2).to(dev)
    labels = torch.randint(0, 125, (B, N), generator=g, dtype=torch.int32).to(dev)
    frame = torch.full((B,), L - 1, dtype=torch.int32, device=dev)
    palette, mean, std = V._device_constants(dev)
    out = [torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev) for _ in range(2)]

    other = ctypes.CDLL(build_nocull())
    ret, kinds = abi.EXT_PROTOTYPES["fod_render_boxes"]
    other.fod_render_boxes.restype, other.fod_render_boxes.argtypes = abi.CTYPE[ret], [abi.CTYPE[k] for k in kinds]
    sb, sl = video.stride()[:2]

    def culled():
        ops.render_boxes(video, boxes, labels, frame_idx=frame, mean=mean, std=std, palette=palette, out=out[0])

    def unculled():
        rc = other.fod_render_boxes(video.data_ptr(), 0, out[1].data_ptr(), B, L, H, W, sb, sl, frame.data_ptr(),
                                    mean.data_ptr(), std.data_ptr(), boxes.data_ptr(), labels.data_ptr(), N,
                                    palette.data_ptr(), palette.shape[0], 3, ops.stream())
        assert rc == 0, rc

    for fn in (culled, unculled):
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    assert torch.equal(out[0], out[1]), "the two forms paint different pictures"
    assert torch.equal(out[0].cpu(), V.render(video[:, -1:].cpu(), boxes.cpu(), labels.cpu())), "the CPU form differs"

    def captured(fn):
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

    graphs = {"tile culling": captured(culled), "no culling": captured(unculled)}
    times = {name: [] for name in graphs}
    for _ in range(ROUNDS):                               # alternating: drift hits both alike
        for name, graph in graphs.items():
            times[name].append(block(graph))

    def host(fn, n=5):
        ts = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts
    clip_ms = host(lambda: video.cpu())
    picture_ms = host(lambda: out[0].cpu())

    def end_to_end():
        culled()
        out[0].cpu()
    both_ms = host(end_to_end)

    moved = B * H * W * 15
    lines = [f"command: python tools/measure_render.py   ({torch.cuda.get_device_name(0)})",
             f"fod_render_boxes, f32 clip {B} x {L} x 3 x {H} x {W}, {N} boxes per sample, thickness 3, last frame of each sample",
             f"device events around a captured graph of {BLOCK} launches, {ROUNDS} alternating replays per form; us per launch",
             f"bytes the map needs: {B} x {H} x {W} x (12 read + 3 written) = {moved / 1e6:.1f} MB per launch", ""]
    for name, ts in times.items():
        med = statistics.median(ts)
        lines.append(f"{name:13s} median {med:8.1f} us   min {min(ts):8.1f}   max {max(ts):8.1f}   "
                     f"spread (max - min) {max(ts) - min(ts):6.1f} us   {moved / med / 1e3:7.1f} GB/s of those bytes")
    lines += ["", f"host clock around the call and a device synchronise, {len(clip_ms)} calls each; ms",
              f"video.cpu() of the whole clip ({video.numel() * 4 / 1e6:.0f} MB, what the reference copies): "
              f"median {statistics.median(clip_ms):.2f}   min {min(clip_ms):.2f}   max {max(clip_ms):.2f}",
              f"picture.cpu() ({out[0].numel() / 1e6:.1f} MB uint8): median {statistics.median(picture_ms):.2f}   "
              f"min {min(picture_ms):.2f}   max {max(picture_ms):.2f}",
              f"render + picture.cpu(): median {statistics.median(both_ms):.2f}   min {min(both_ms):.2f}   max {max(both_ms):.2f}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
