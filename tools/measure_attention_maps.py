"""What looking at the attention costs (profiles/attention_maps_cost.txt).

    python tools/measure_attention_maps.py [--out FILE]

1. fod_attn_maps at the headline extent -- B = 2, J = 5 memory images of 29 x 50 = 1450 keys, H = 8, 300 queries, bf16,
   the operands laid out as the decoder's MemorySide lays them out (key slots of a [B, N, 2 * 6 * 256] buffer, one
   positional table for the batch) -- for Q = 100 and Q = 300 selected queries, beside the torch form that was the only
   one before (`_head_mean_weights` on each of the five blocks, all 300 queries), and against the bytes the launch
   needs: two passes over the keys plus the output.  The kernel's launches are captured into a hipGraph (one launch is
   shorter than the Python around it); the torch form is a dozen launches per block and is timed as it is called.
2. fod_render_attention at 2 x 5 pictures of 900 x 1600 beside what the reference's notebook does with one detection's
   maps: F.interpolate to full size and `.cpu()`.
A measurement needs the GPU: without one this fails."""
import argparse
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "future-object-detection_amd")
sys.path[:0] = [ROOT, PKG]

import torch  # noqa: E402

B, J, MH, MW, HEADS, D, M, LAYERS = 2, 5, 29, 50, 8, 256, 300, 6
L, H, W = 6, 900, 1600
BLOCK, ROUNDS = 50, 12


def events(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n                      # us per call


def host(fn, n=5):
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def row(name, ts, unit="us"):
    return f"{name:44s} median {statistics.median(ts):9.1f} {unit}   min {min(ts):9.1f}   max {max(ts):9.1f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    import torch.nn.functional as F
    from future_od.models.transformer import _head_mean_weights
    from future_od.native import ops
    from future_od.utils import visualization as V
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    N = MH * MW
    rnd = lambda *shape: torch.randn(*shape, generator=g).to(dev, torch.bfloat16)
    big = [rnd(B, N, 2 * LAYERS * D) for _ in range(J)]
    ks_all = rnd(N, LAYERS * J * D)
    last = LAYERS - 1
    jobs = []
    for j in range(J):
        kc = big[j][..., (2 * last + 1) * D:(2 * last + 2) * D]
        ks = ks_all[..., (last * J + j) * D:(last * J + j + 1) * D]
        jobs.append((rnd(B, M, D), rnd(B, M, D), kc, ks))
    scale = 1.0 / math.sqrt(2 * D // HEADS)
    idx = {Q: torch.stack([torch.randperm(M, generator=g)[:Q] for _ in range(B)]).to(dev, torch.int32) for Q in (100, 300)}
    outs = {Q: torch.empty(B, Q, J, N, dtype=torch.float32, device=dev) for Q in idx}

    def torch_form():
        return [_head_mean_weights(qc, kc, qs, ks.unsqueeze(0).expand(B, -1, -1), HEADS) for qc, qs, kc, ks in jobs]

    for Q in idx:
        ops.attn_maps(jobs, scale, idx[Q], out=outs[Q])
    want = torch.stack(torch_form(), dim=2)                                        # [B, M, J, N]
    torch.cuda.synchronize()
    for Q in idx:
        picked = torch.gather(want, 1, idx[Q].long()[:, :, None, None].expand(-1, -1, J, N))
        err = float(((outs[Q] - picked).abs() / picked.amax(-1, keepdim=True)).max())
        assert err < 1e-4, (Q, err)

    graphs = {}
    for Q in idx:
        graphs[Q] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[Q]):
            for _ in range(BLOCK):
                ops.attn_maps(jobs, scale, idx[Q], out=outs[Q])
        graphs[Q].replay()
    for _ in range(3):
        torch_form()
    torch.cuda.synchronize()
    times = {"fod_attn_maps Q = 100": [], "fod_attn_maps Q = 300": [], "torch, five blocks x 300 queries": []}
    for _ in range(ROUNDS):                                                        # alternating: drift hits all alike
        times["fod_attn_maps Q = 100"].append(events(graphs[100].replay, 1) / BLOCK)
        times["fod_attn_maps Q = 300"].append(events(graphs[300].replay, 1) / BLOCK)
        times["torch, five blocks x 300 queries"].append(events(torch_form, 10))
    key_bytes = J * (B * N * D * 2 + N * D * 2)                                    # content keys per sample, one table
    lines = [f"command: python tools/measure_attention_maps.py   ({torch.cuda.get_device_name(0)})", "",
             f"1. fod_attn_maps: B {B}, J {J} images of {MH} x {MW} = {N} keys, H {HEADS}, {M} queries, bf16, slot-strided keys",
             f"   kernel: device events around a captured graph of {BLOCK} launches; torch: events around 10 eager calls of the",
             f"   five blocks (`_head_mean_weights`, what store_attention ran before); {ROUNDS} alternating rounds; us per call", ""]
    for name, ts in times.items():
        lines.append("   " + row(name, ts))
    lines.append("")
    for Q in idx:
        need = 2 * key_bytes + B * Q * J * N * 4
        med = statistics.median(times[f"fod_attn_maps Q = {Q}"])
        flop = 2 * 2.0 * J * B * HEADS * Q * N * 64
        lines.append(f"   Q = {Q}: the launch needs 2 x {key_bytes / 1e6:.2f} MB of keys + {B * Q * J * N * 4 / 1e6:.2f} MB of maps = "
                     f"{need / 1e6:.2f} MB: {need / med / 1e3:.0f} GB/s of those bytes, {flop / med / 1e6:.2f} TFLOP/s of its "
                     f"{flop / 1e9:.2f} GFLOP (both passes)")
    tmed = statistics.median(times["torch, five blocks x 300 queries"])
    for Q in idx:
        lines.append(f"   torch / kernel at Q = {Q}: {tmed / statistics.median(times[f'fod_attn_maps Q = {Q}']):.1f} x")

    # ---- 2. the overlay
    video = torch.randn(B, L, 3, H, W, generator=g).to(dev)
    att = outs[100].view(B, 100, J, MH, MW)
    frames = torch.arange(L - 2, L - 2 - J, -1, dtype=torch.int32)
    pictures = V.render_attention(video, att, frames, 0)
    assert tuple(pictures.shape) == (B, J, H, W, 3)
    sample = V.render_attention(video[:1, :, :, :90, :160].contiguous().cpu(), att[:1].cpu(), frames, 0)
    small = V.render_attention(video[:1, :, :, :90, :160].contiguous(), att[:1], frames, 0)
    assert torch.equal(small.cpu(), sample), "the CPU form differs"
    maps = att[:, 0]

    def reference_way():
        return F.interpolate(maps, size=(H, W), mode="bilinear", align_corners=False).cpu()

    def ours():
        return V.render_attention(video, att, frames, 0).cpu()

    for _ in range(3):
        V.render_attention(video, att, frames, 0)
    torch.cuda.synchronize()
    dev_us = [events(lambda: V.render_attention(video, att, frames, 0), 10) for _ in range(ROUNDS)]
    ref_ms, our_ms = [], []
    for _ in range(5):
        ref_ms += host(reference_way, 1)
        our_ms += host(ours, 1)
    moved = B * J * H * W * 15
    lines += ["", f"2. fod_render_attention: {B} x {J} pictures of {H} x {W} from an f32 clip, maps {MH} x {MW}, one detection per sample",
              f"   device events around 10 calls of visualization.render_attention (the launch and four tiny torch ops), {ROUNDS} rounds",
              "   " + row("render_attention on the device", dev_us),
              f"   bytes the map needs: {B * J} x {H} x {W} x (12 read + 3 written) = {moved / 1e6:.0f} MB: "
              f"{moved / statistics.median(dev_us) / 1e3:.0f} GB/s of those bytes",
              "   host clock around the call and a device synchronise, 5 alternating calls each; ms",
              "   " + row(f"F.interpolate to full size + .cpu() ({B * J * H * W * 4 / 1e6:.0f} MB f32)", ref_ms, "ms"),
              "   " + row(f"render_attention + .cpu() ({B * J * H * W * 3 / 1e6:.0f} MB uint8)", our_ms, "ms")]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
