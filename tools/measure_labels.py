"""What captions cost (profiles/render_labels_cost.txt): fod_render_labels with 100 and with 300 captions per sample on
2 x 900 x 1600 pictures at scale 2, beside fod_render_boxes producing those pictures from an f32 clip with the same
boxes, in the same trace, and beside a launch whose labels are all hidden (what reading the labels alone costs).

    python tools/measure_labels.py [--out FILE]

Every caption carries all three parts ("<query> <name> <percent>", the names of a driving data set).  A block of
launches of each kernel is captured into a hipGraph (the launching thread's Python per call would otherwise be part of
what is timed), and the graphs are replayed in alternation between device events, so the spread between blocks of ONE
kernel is seen beside the difference between them.  The pictures are compared with the CPU form byte for byte first.
The bytes fod_render_labels has to move are the plate pixels it writes (3 B each; counted by painting on two different
backgrounds and keeping the pixels that agree) and the labels every block reads.  A measurement needs the GPU: without
one this fails."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "future-object-detection_amd")
sys.path[:0] = [ROOT, PKG]

import torch  # noqa: E402

B, L, H, W, BLOCK, ROUNDS, SCALE = 2, 6, 900, 1600, 400, 12, 2
COUNTS = (100, 300)
NAMES = ["car", "truck", "bus", "trailer", "construction_vehicle", "pedestrian", "motorcycle", "bicycle", "traffic_cone",
         "barrier"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    from future_od.native import ops
    from future_od.utils import visualization as V
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    video = torch.randn(B, L, 3, H, W, generator=g).to(dev)
    frame = torch.full((B,), L - 1, dtype=torch.int32, device=dev)
    palette, mean, std = V._device_constants(dev)
    captions = V.Captions(names=[NAMES[i % len(NAMES)] for i in range(125)], scale=SCALE)    # every class has a name
    names, font = captions.tables(dev)
    out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev)

    def operands(n):
        wh = torch.rand(B, n, 2, generator=g) * torch.tensor([W * 0.3, H * 0.3]) + 8.0
        xy = torch.rand(B, n, 2, generator=g) * (torch.tensor([float(W), float(H)]) - wh)
        return dict(boxes=torch.cat([xy, xy + wh], dim=2).to(dev),
                    labels=torch.randint(0, 125, (B, n), generator=g, dtype=torch.int32).to(dev),
                    idents=torch.randint(0, 1024, (B, n), generator=g, dtype=torch.int32).to(dev),
                    scores=torch.rand(B, n, generator=g).to(dev))

    def boxes_fn(o):
        return lambda: ops.render_boxes(video, o["boxes"], o["labels"], frame_idx=frame, mean=mean, std=std,
                                        palette=palette, out=out)

    def labels_fn(o, pictures=out):
        return lambda: ops.render_labels(pictures, o["boxes"], o["labels"], idents=o["idents"], scores=o["scores"],
                                         names=names, palette=palette, font=font, scale=SCALE)

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

    lines = [f"command: python tools/measure_labels.py   ({torch.cuda.get_device_name(0)})",
             f"pictures {B} x {H} x {W} x 3 uint8 from an f32 clip {B} x {L} x 3 x {H} x {W}; captions \"<query> <name> "
             f"<percent>\", 5x7 font, scale {SCALE}, thickness 3",
             f"device events around a captured graph of {BLOCK} launches, {ROUNDS} alternating replays per kernel; us per launch",
             ""]
    graphs, moved = {}, {}
    for n in COUNTS:
        o = operands(n)
        boxes_fn(o)()
        labels_fn(o)()
        torch.cuda.synchronize()
        want = V.render(video[:, -1:].cpu(), o["boxes"].cpu(), o["labels"].cpu(),
                        captions=captions.replace(ident=o["idents"].cpu(), scores=o["scores"].cpu()))
        assert torch.equal(out.cpu(), want), "the CPU form differs"
        painted = []
        for fill in (0x00, 0xFF):
            canvas = torch.full_like(out, fill)
            labels_fn(o, canvas)()
            painted.append(canvas)
        torch.cuda.synchronize()
        pixels = int((painted[0] == painted[1]).all(dim=3).sum())
        tiles = B * ((W + 255) // 256) * ((H + 15) // 16)
        moved[n] = (pixels, 3 * pixels + tiles * n * 28)
        graphs[f"fod_render_boxes, {n} boxes"] = (captured(boxes_fn(o)), B * H * W * 15)
        graphs[f"fod_render_labels, {n} captions"] = (captured(labels_fn(o)), moved[n][1])
        if n == COUNTS[-1]:                               # the floor: every block reads the labels and finds none to draw
            hidden = dict(o, labels=torch.full_like(o["labels"], -1))
            graphs[f"fod_render_labels, {n} labels, none drawn"] = (captured(labels_fn(hidden)), tiles * n * 4)
    times = {name: [] for name in graphs}
    for _ in range(ROUNDS):                               # alternating: drift hits all alike
        for name, (graph, _) in graphs.items():
            times[name].append(block(graph))
    lines.append(f"bytes fod_render_boxes needs: {B} x {H} x {W} x (12 read + 3 written) = {B * H * W * 15 / 1e6:.1f} MB per launch")
    for n in COUNTS:
        pixels, nbytes = moved[n]
        lines.append(f"bytes fod_render_labels needs with {n} captions: {pixels} plate pixels x 3 written "
                     f"({100.0 * pixels / (B * H * W):.1f} % of the pictures) + {n} labels x 28 read by each of "
                     f"{B * ((W + 255) // 256) * ((H + 15) // 16)} blocks = {nbytes / 1e6:.2f} MB per launch")
    lines.append("")
    for name, ts in times.items():
        med = statistics.median(ts)
        lines.append(f"{name:42s} median {med:8.1f} us   min {min(ts):8.1f}   max {max(ts):8.1f}   "
                     f"spread (max - min) {max(ts) - min(ts):6.1f} us   {graphs[name][1] / med / 1e3:7.1f} GB/s of those bytes")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
