"""What does the frame-windowed self-attention launch (csrc/attn7p.hip, icv_attention_fwd_framewin) cost at the 14B / 480p
shape?  T = 21 latent frames of F = 1 560 tokens, 40 heads, unit scale, window = 4, sink = 1.  Three things, interleaved in one process:
  (a) the ONE frame-windowed launch;
  (b) the 21 per-frame icv_attention_fwd_pieces launches it replaces (same tiles, same bits - checked here);
  (c) the dense icv_attention_fwd launch.
Every variant is warmed up; a round times ITERS back-to-back calls of each variant between device events (0.4 - 0.8 s per timed window
at the defaults), the order of the variants alternates from round to round, and the median over the rounds is reported with every
round's value next to it.  host_enqueue_ms is the wall-clock time the host needs to enqueue one call (for (b): building and passing 21
piece arrays), taken on one call into an empty queue before each timed window: a variant whose host time is below its device time is
bound by the device, not by the enqueue.  Run on the GPU box:
    python tools/attn_framewin_study.py --out profiles/attn_framewin_study.json"""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from infinicube_amd.videogen import attn_window as AW  # noqa: E402
from infinicube_amd.videogen.ops import HipOps  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=21)
    ap.add_argument("--frame-rows", type=int, default=1560)
    ap.add_argument("--heads", type=int, default=40)
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--sink", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_framewin_study: no GPU - a timing taken anywhere else says nothing")
    ops = HipOps("cuda:0")
    T, F, H = a.frames, a.frame_rows, a.heads
    S, d, scale = T * F, H * 128, math.log(2.0)
    torch.manual_seed(0)
    qkv = torch.randn((3, S, d), device="cuda").to(torch.bfloat16)
    qkv[1] = (qkv[1].float() * (128 ** -0.5 * math.log2(math.e))).to(torch.bfloat16)      # the DiT's K: softmax scale and log2(e) folded in
    q, k, v = qkv[0], qkv[1], qkv[2]
    oa, ob, oc = torch.empty_like(q), torch.empty_like(q), torch.empty_like(q)
    ranges = AW.ranges(T, a.window, a.sink)
    pieces = [[(k[r0 * F: r1 * F], v[r0 * F: r1 * F], -1, 0) for r0, r1 in rs] for rs in ranges]

    def one_launch():
        ops.attention_framewin(q, k, v, oa, H, scale, T, F, a.window, a.sink)

    def per_frame():
        for f in range(T):
            ops.attention_pieces(q[f * F: (f + 1) * F], pieces[f], ob[f * F: (f + 1) * F], H, scale)

    def dense():
        ops.attention(q, k, v, oc, H, scale)

    variants = [("framewin_one_launch", one_launch), ("pieces_per_frame", per_frame), ("dense", dense)]
    for _, fn in variants:
        fn()
        fn()
    torch.cuda.synchronize()
    same = bool(torch.equal(oa, ob))
    times = {name: [] for name, _ in variants}
    host = {name: [] for name, _ in variants}
    for r in range(a.rounds):
        order = variants if r % 2 == 0 else variants[::-1]
        for name, fn in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            h0 = time.perf_counter()                 # one call into an empty queue: what the host spends enqueueing it
            fn()
            host[name].append((time.perf_counter() - h0) * 1e3)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.iters)
    med = {name: sorted(ts)[len(ts) // 2] for name, ts in times.items()}
    host_med = {name: sorted(ts)[len(ts) // 2] for name, ts in host.items()}
    kf = AW.key_fraction(T, a.window, a.sink)
    bpf = -(-F // 256)
    res = dict(shape=dict(frames=T, frame_rows=F, heads=H, S=S, window=a.window, sink=a.sink, scale="unit (ln 2)"),
               key_fraction=kf, q_block_fill=F / (256.0 * bpf), work_groups=H * T * bpf,
               bit_identical_to_per_frame_launches=same, rounds=a.rounds, iters_per_round=a.iters,
               median_ms=med, host_enqueue_ms={n: round(x, 4) for n, x in host_med.items()}, rounds_ms={n: [round(x, 4) for x in ts] for n, ts in times.items()},
               one_launch_over_per_frame=med["framewin_one_launch"] / med["pieces_per_frame"],
               one_launch_over_dense=med["framewin_one_launch"] / med["dense"],
               estimate_one_launch_over_dense=kf * 256.0 * bpf / F,
               dense_tflops=4.0 * S * S * d / med["dense"] / 1e9, one_launch_tflops=4.0 * S * S * d * kf / med["framewin_one_launch"] / 1e9)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    if not same:
        raise SystemExit("attn_framewin_study: the one launch and the per-frame launches differ")


if __name__ == "__main__":
    main()
