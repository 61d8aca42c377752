"""What radial self-attention costs (run on the GPU box), in two parts.

Kernels (--out-kernels): the 14B / 480p self-attention, (T, F, H) = (21, 1560, 40) bf16 at the DiT's folded scale, in ONE process: the
dense launch (icv_attention_fwd), the frame window 4 + 1 anchor frame (icv_attention_fwd_framewin) and radial 1 + 1
(icv_attention_fwd_radial), the three alternating, warm, each launch between its own pair of device events, the median of --launches
launches.  Next to the times: the share of (query row, key row) pairs each launch reads and the 64-key tiles it issues per head,
counted on the host (attn_window.radial_key_fraction / radial_tiles / framewin_tiles).

Steps (--out-step): at synthetic weights of --model, 93 frames 480 x 832, bf16, cfg_scale = 5, after --warm-steps steps the median of
--steps steps of (a) dense attention, (b) the frame window, (c) radial.

Each part is a GPU step of its own - give each its own time limit:

    timeout -k 10 300 python tools/radial_attention_bench.py --skip-step --out-kernels profiles/radial_attention.json
    timeout -k 10 600 python tools/radial_attention_bench.py --skip-kernels --out-step profiles/radial_attention_step.json
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from infinicube_amd.videogen import attn_window as AW  # noqa: E402
from infinicube_amd.videogen import synthetic as syn  # noqa: E402
from infinicube_amd.videogen.config import GRID_480P, TokenGrid, preset  # noqa: E402
from infinicube_amd.videogen.dit import WanDiT  # noqa: E402
from infinicube_amd.videogen.ops import HipOps  # noqa: E402
from infinicube_amd.videogen.scheduler import FlowMatchScheduler  # noqa: E402

DEV = "cuda:0"
WINDOW, RADIAL = (4, 1), (1, 1)         # (window, sink) of the frame-window arm and of the radial arm


def write(path, result):
    print(json.dumps(result), flush=True)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


def kernels(ops, args):
    T, F, H = args.T, args.F, args.heads
    g = torch.Generator().manual_seed(T * F)
    q, k, v = (torch.randn((T * F, H * 128), generator=g).to(torch.bfloat16).to(DEV) for _ in range(3))
    k = (k.float() * (math.log2(math.e) / math.sqrt(128))).to(torch.bfloat16)         # the DiT's fold: scale * log2(e) in K, scale = ln 2
    o = torch.empty_like(q)
    scale = math.log(2.0)
    fns = {"dense": lambda: ops.attention(q, k, v, o, H, scale),
           "framewin": lambda: ops.attention_framewin(q, k, v, o, H, scale, T, F, *WINDOW),
           "radial": lambda: ops.attention_radial(q, k, v, o, H, scale, T, F, *RADIAL)}
    times = {name: [] for name in fns}
    for i in range(args.warmup + args.launches):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                times[name].append(e0.elapsed_time(e1))
    host = {"dense": dict(key_fraction=1.0, tiles_per_head=-(-T * F // 256) * -(-T * F // 64)),     # its q-blocks tile all rows, not a frame's
            "framewin": dict(window=WINDOW[0], sink=WINDOW[1], key_fraction=round(AW.key_fraction(T, *WINDOW), 4),
                             tiles_per_head=AW.framewin_tiles(T, F, *WINDOW)),
            "radial": dict(window=RADIAL[0], sink=RADIAL[1], key_fraction=round(AW.radial_key_fraction(T, F, *RADIAL), 4),
                           radial_tiles=AW.radial_tiles(T, F, *RADIAL), tiles_per_head=AW.radial_tiles(T, F, *RADIAL),
                           max_pieces=AW.radial_record(T, F, *RADIAL)["max_pieces"])}
    result = dict(what="ms per launch, one pair of device events per launch, warm, the three launches alternating in one process; key_fraction and "
                       "tiles_per_head (64-key tiles, summed over the (frame, 256-row block) work-groups of one head) are counted on the host",
                  launches=args.launches, warmup=args.warmup, device=torch.cuda.get_device_name(0), frames=T, frame_rows=F, heads=H, dtype="bf16",
                  scale="folded (unit)", arms={})
    for name, t in times.items():
        result["arms"][name] = dict(median_ms=round(statistics.median(t), 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4), **host[name])
    a = result["arms"]
    result["radial_over_dense"] = round(a["radial"]["median_ms"] / a["dense"]["median_ms"], 4)
    result["radial_over_framewin"] = round(a["radial"]["median_ms"] / a["framewin"]["median_ms"], 4)
    result["radial_tiles_over_framewin_tiles"] = round(a["radial"]["tiles_per_head"] / a["framewin"]["tiles_per_head"], 4)
    write(args.out_kernels, result)


def steps(ops, args):
    cfg, grid = preset(args.model), TokenGrid(args.frames, args.height, args.width)
    sd = syn.make_dit_state_dict(cfg, seed=0, device=DEV, dtype=torch.bfloat16)
    bsd = syn.make_buffer_embedder_state_dict(cfg, device=DEV, dtype=torch.bfloat16)
    model = WanDiT(cfg, sd, ops, bsd)
    del sd, bsd
    model.prepare(grid, graphs=False)
    ctx_c, ctx_u = model.encode_context(syn.make_text_context(cfg, 1)), model.encode_context(syn.make_text_context(cfg, 2))
    buf = model.embed_buffers(syn.make_buffer_latents(cfg, grid))
    sched = FlowMatchScheduler(50)
    n = args.warm_steps + args.steps
    T, F = grid.T, grid.tokens_per_frame
    arms = (("dense", None), ("framewin", WINDOW + (False,)), ("radial", RADIAL + (True,)))
    result = dict(what=f"seconds per denoising step (two forwards, cfg_scale = 5), median of {args.steps} after {args.warm_steps} warm steps, host clock "
                       "around a synchronised step", model=args.model, frames=args.frames, height=args.height, width=args.width, tokens=grid.S,
                  latent_frames=T, frame_rows=F, layers=cfg.num_layers, dtype="bf16", data="synthetic weights and inputs",
                  device=torch.cuda.get_device_name(0), arms={})
    for name, setting in arms:
        if setting is None:
            model.set_attention_window(None, None)
        else:
            model.set_attention_window(setting[0], setting[1], radial=setting[2])
        latent = syn.make_latent_noise(grid, seed=0).to(DEV)
        marks = []

        def on_step(i, lat):
            torch.cuda.synchronize()
            marks.append(time.perf_counter())

        torch.cuda.synchronize()
        marks.append(time.perf_counter())
        model.denoise(latent, ctx_c, ctx_u, buf, sched, 5.0, steps=range(n), on_step=on_step)
        per = [b - a for a, b in zip(marks[:-1], marks[1:])][args.warm_steps:]
        assert bool(torch.isfinite(latent).all())
        result["arms"][name] = dict(median_s=round(statistics.median(per), 4), min_s=round(min(per), 4), max_s=round(max(per), 4))
        if setting is not None:
            result["arms"][name].update(window=setting[0], sink=setting[1], key_fraction=round(
                AW.radial_key_fraction(T, F, *setting[:2]) if setting[2] else AW.key_fraction(T, *setting[:2]), 4))
        print(name, result["arms"][name], flush=True)
    a = result["arms"]
    result["radial_step_over_dense_step"] = round(a["radial"]["median_s"] / a["dense"]["median_s"], 4)
    result["radial_step_over_framewin_step"] = round(a["radial"]["median_s"] / a["framewin"]["median_s"], 4)
    write(args.out_step, result)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("-T", type=int, default=21)
    ap.add_argument("-F", type=int, default=1560)
    ap.add_argument("--heads", type=int, default=40)
    ap.add_argument("--model", default="14b", choices=["14b", "1.3b", "small", "tiny"])
    ap.add_argument("--frames", type=int, default=GRID_480P.num_frames)
    ap.add_argument("--height", type=int, default=GRID_480P.height)
    ap.add_argument("--width", type=int, default=GRID_480P.width)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warm-steps", type=int, default=2)
    ap.add_argument("--out-kernels", default=None)
    ap.add_argument("--out-step", default=None)
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    ops = HipOps(DEV)
    if not args.skip_kernels:
        kernels(ops, args)
    if not args.skip_step:
        steps(ops, args)


if __name__ == "__main__":
    main()
