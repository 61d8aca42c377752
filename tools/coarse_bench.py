"""What coarse-to-fine sampling costs and saves (run on the GPU box), in two parts.

Kernels (--out-kernels): icv_latent_resize_noise_f32 on 16 x 21 planes at 60 x 104 -> 90 x 160 (the 480p coarse stage of a 720p call)
and 30 x 52 -> 60 x 104 (the 240p coarse stage of a 480p call), next to icv_add_noise_f32 at each OUTPUT size from the same process.
Warm, the kernels alternating, each launch between its own pair of device events, the median of --launches launches.

Steps (--out-step): at synthetic weights of --model, 93 frames, bf16, cfg_scale = 5, after --warm-steps steps the median of --steps
steps of the plain loop at 480 x 832, on the coarse twin (WanDiT.coarse_engine) at 240 x 416 and - unless --skip-720p, or when its
workspace does not fit - on a second workspace at 720 x 1280.  The loops alternate --rounds times in the one process; per-round figures
and the pooled medians are written.  With --plain-only only the 480 x 832 loop runs and nothing of the feature is touched: that is how
the parent commit's plain step is timed from its own checkout in the same session (--parent-step adds its file to the result).

    python tools/coarse_bench.py --out-kernels profiles/coarse_kernels.json --out-step profiles/coarse_step.json
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from infinicube_amd.videogen import synthetic as syn  # noqa: E402
from infinicube_amd.videogen.config import TokenGrid, preset  # noqa: E402
from infinicube_amd.videogen.dit import WanDiT  # noqa: E402
from infinicube_amd.videogen.ops import HipOps  # noqa: E402
from infinicube_amd.videogen.scheduler import FlowMatchScheduler  # noqa: E402

DEV = "cuda:0"


def write(path, result):
    print(json.dumps(result), flush=True)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


def kernels(ops, args):
    g = torch.Generator().manual_seed(1)
    sigma = FlowMatchScheduler(50).sigmas[25]
    fns, moved = {}, {}
    for (h_in, w_in), (h_out, w_out) in (((60, 104), (90, 160)), ((30, 52), (60, 104))):
        x0 = torch.randn((16, 21, h_in, w_in), generator=g).to(DEV)
        noise, x_same, out = (torch.randn((16, 21, h_out, w_out), generator=g).to(DEV) for _ in range(3))
        tag = f"{h_in}x{w_in} -> {h_out}x{w_out}"
        fns[f"icv_latent_resize_noise_f32 {tag}"] = lambda x0=x0, noise=noise: ops.latent_resize_noise(x0, noise, sigma)
        fns[f"icv_add_noise_f32 {h_out}x{w_out}"] = lambda x=x_same, z=noise, o=out: ops.add_noise(x, z, o, sigma)
        # bytes: the switch reads x0 once (its four taps per output hit cache) and reads + writes the output; add_noise reads two, writes one
        moved[f"icv_latent_resize_noise_f32 {tag}"] = 4 * (x0.numel() + 2 * noise.numel())
        moved[f"icv_add_noise_f32 {h_out}x{w_out}"] = 4 * 3 * noise.numel()
    times = {name: [] for name in fns}
    for it in range(args.warmup + args.launches):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    result = dict(what="time per launch, one pair of device events per launch, warm, the kernels alternating in one process; normal draws; "
                       "the switch runs in place over its output again and again (the values drift, the work does not)",
                  planes=[16, 21], launches=args.launches, warmup=args.warmup, device=torch.cuda.get_device_name(0), kernels={})
    for name, t in times.items():
        med = statistics.median(t)
        result["kernels"][name] = dict(median_us=round(med, 2), min_us=round(min(t), 2), max_us=round(max(t), 2), bytes=moved[name],
                                       gb_per_s_at_median=round(moved[name] / med / 1e3, 1))
    write(args.out_kernels, result)


def steps(ops, args):
    cfg = preset(args.model)
    fine, coarse, large = TokenGrid(args.frames, 480, 832), TokenGrid(args.frames, 240, 416), TokenGrid(args.frames, 720, 1280)
    sd = syn.make_dit_state_dict(cfg, seed=0, device=DEV, dtype=torch.bfloat16)
    bsd = syn.make_buffer_embedder_state_dict(cfg, device=DEV, dtype=torch.bfloat16)
    model = WanDiT(cfg, sd, ops, bsd)
    del sd, bsd
    model.prepare(fine, graphs=False)
    ctx_c, ctx_u = model.encode_context(syn.make_text_context(cfg, 1)), model.encode_context(syn.make_text_context(cfg, 2))
    sched = FlowMatchScheduler(50)
    result = dict(what=f"seconds per denoising step, median of {args.steps} after {args.warm_steps} warm steps, host clock around a synchronised step",
                  model=args.model, frames=args.frames, layers=cfg.num_layers, dtype="bf16", cfg_scale=5.0, data="synthetic weights and inputs",
                  device=torch.cuda.get_device_name(0), arms={}, missing=[])
    engines = {"480x832": (model, fine)}
    if not args.plain_only:
        free0 = torch.cuda.mem_get_info()[0]
        engines["240x416"] = (model.coarse_engine(coarse.height, coarse.width), coarse)
        torch.cuda.synchronize()
        result["coarse_twin_workspace_bytes_240x416"] = int(free0 - torch.cuda.mem_get_info()[0])      # by the allocator's free memory
        if not args.skip_720p:
            try:
                engines["720x1280"] = (model._engine_copy().prepare(large, graphs=False), large)
            except torch.OutOfMemoryError as e:
                result["missing"].append(f"720x1280 step: the workspace did not fit ({str(e)[:80]})")
        else:
            result["missing"].append("720x1280 step: not run (--skip-720p)")
    bufs = {name: eng.embed_buffers(syn.make_buffer_latents(cfg, grid)) for name, (eng, grid) in engines.items()}
    result["tokens"] = {name: grid.S for name, (_, grid) in engines.items()}

    def run(name, n):
        eng, grid = engines[name]
        latent = syn.make_latent_noise(grid, seed=0).to(DEV)
        marks = []

        def on_step(i, lat):
            torch.cuda.synchronize()
            marks.append(time.perf_counter())

        torch.cuda.synchronize()
        marks.append(time.perf_counter())
        eng.denoise(latent, ctx_c, ctx_u, bufs[name], sched, 5.0, steps=range(n), on_step=on_step)
        assert bool(torch.isfinite(latent).all())
        return [b - a for a, b in zip(marks[:-1], marks[1:])]

    def arm(name, per):
        result["arms"][name] = dict(median_s=round(statistics.median(per), 4), min_s=round(min(per), 4), max_s=round(max(per), 4), steps=len(per))
        print(name, result["arms"][name], flush=True)

    pooled = {name: [] for name in engines}
    for r in range(args.rounds):                      # the loops alternate in this one process; every loop starts with its own warm steps
        for name in engines:
            per = run(name, args.warm_steps + args.steps)[args.warm_steps:]
            pooled[name] += per
            arm(f"{name}, round {r + 1}", per)
    for name, per in pooled.items():
        arm(name, per)
    a = result["arms"]
    if "240x416" in a:
        result["coarse_step_over_fine_step"] = round(a["240x416"]["median_s"] / a["480x832"]["median_s"], 4)
    if "720x1280" in a:
        result["480p_step_over_720p_step"] = round(a["480x832"]["median_s"] / a["720x1280"]["median_s"], 4)
    if args.parent_step:
        with open(args.parent_step) as f:
            a["parent commit, 480x832"] = json.load(f)["arms"]["480x832"]
        result["plain_step_over_parent_plain_step"] = round(a["480x832"]["median_s"] / a["parent commit, 480x832"]["median_s"], 4)
    write(args.out_step, result)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--model", default="14b", choices=["14b", "1.3b", "small", "tiny"])
    ap.add_argument("--frames", type=int, default=93)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warm-steps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2, help="how often the step loops alternate")
    ap.add_argument("--out-kernels", default=None)
    ap.add_argument("--out-step", default=None)
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-720p", action="store_true")
    ap.add_argument("--plain-only", action="store_true", help="time the plain 480 x 832 step only; touches nothing of the feature (a parent checkout)")
    ap.add_argument("--parent-step", default=None, help="the --out-step file of a --plain-only run from the parent commit's checkout")
    args = ap.parse_args()
    ops = HipOps(DEV)
    if not args.skip_kernels:
        kernels(ops, args)
    if not args.skip_step:
        steps(ops, args)


if __name__ == "__main__":
    main()
