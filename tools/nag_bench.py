"""What Normalized Attention Guidance costs (run on the GPU box), in two parts.

Kernels (--out-kernels): icv_nag_combine_bf16 in place at 37 440 x 5120 and 32 760 x 1536, next to icv_ln_modulate at the same shape
from the same process - a kernel of the same structure (row in registers, row reductions, one write) that moves the same 6 bytes per
element.  Warm, the two alternating, each launch between its own pair of device events, the median of --launches launches; bytes moved
divided by time for both.

Steps (--out-step): at synthetic weights of --model, 93 frames 480 x 832, bf16, after --warm-steps steps the median of --steps steps of
(a) cfg_scale = 5, the two-forward step; (b) cfg_scale = 1, one forward; (c) cfg_scale = 1 with NAG.

    python tools/nag_bench.py --out-kernels profiles/nag_kernels.json --out-step profiles/nag_step.json
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
from infinicube_amd.videogen.config import GRID_480P, TokenGrid, preset  # noqa: E402
from infinicube_amd.videogen.dit import WanDiT  # noqa: E402
from infinicube_amd.videogen.nag import NagPlan  # noqa: E402
from infinicube_amd.videogen.ops import HipOps  # noqa: E402
from infinicube_amd.videogen.scheduler import FlowMatchScheduler  # noqa: E402

DEV = "cuda:0"
NAG = (11.0, 2.5, 0.25)


def write(path, result):
    print(json.dumps(result), flush=True)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


def kernels(ops, args):
    result = dict(what="time per launch, one pair of device events per launch, warm, the two kernels alternating in one process; bytes = 6 per "
                       "element for both (nag_combine: two bf16 reads + one bf16 write; ln_modulate: one f32 read + one bf16 write)",
                  launches=args.launches, warmup=args.warmup, device=torch.cuda.get_device_name(0), nag=list(NAG), shapes=[])
    for rows, d in ((37440, 5120), (32760, 1536)):
        g = torch.Generator().manual_seed(rows)
        p0 = torch.randn((rows, d), generator=g).to(torch.bfloat16).to(DEV)
        zn = (p0.float() + 0.25 * torch.randn((rows, d), generator=g).to(DEV)).to(torch.bfloat16)
        zp = p0.clone()
        x = torch.randn((rows, d), generator=g).to(DEV)
        h = torch.empty((rows, d), dtype=torch.bfloat16, device=DEV)
        shift, scale = torch.randn(d, generator=g).to(DEV), torch.randn(d, generator=g).to(DEV)
        fns = {"icv_nag_combine_bf16": lambda: ops.nag_combine(zp, zn, zp, *NAG),
               "icv_ln_modulate": lambda: ops.ln_modulate(x, h, shift=shift, scale=scale, eps=1e-6)}
        times = {k: [] for k in fns}
        for k in range(args.warmup + args.launches):
            zp.copy_(p0)                                                          # the combine runs in place: start every launch from z+
            for name, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if k >= args.warmup:
                    times[name].append(e0.elapsed_time(e1) * 1e3)
        row = dict(rows=rows, d=d, bytes=6 * rows * d, kernels={})
        for name, t in times.items():
            med = statistics.median(t)
            row["kernels"][name] = dict(median_us=round(med, 2), min_us=round(min(t), 2), max_us=round(max(t), 2),
                                        gb_per_s_at_median=round(6 * rows * d / med / 1e3, 1))
        k = row["kernels"]
        row["nag_over_ln_modulate_bandwidth"] = round(k["icv_nag_combine_bf16"]["gb_per_s_at_median"] / k["icv_ln_modulate"]["gb_per_s_at_median"], 3)
        result["shapes"].append(row)
        del p0, zn, zp, x, h
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
    arms = (("cfg_scale=5", dict(ctx_uncond=ctx_u, cfg_scale=5.0)), ("cfg_scale=1", dict(ctx_uncond=None, cfg_scale=1.0)),
            ("cfg_scale=1+nag", dict(ctx_uncond=None, cfg_scale=1.0, nag=NagPlan(ctx_u, *NAG))))
    result = dict(what=f"seconds per denoising step, median of {args.steps} after {args.warm_steps} warm steps, host clock around a synchronised step",
                  model=args.model, frames=args.frames, height=args.height, width=args.width, tokens=grid.S, layers=cfg.num_layers, dtype="bf16",
                  data="synthetic weights and inputs", device=torch.cuda.get_device_name(0), nag=list(NAG), arms={})
    for name, kw in arms:
        latent = syn.make_latent_noise(grid, seed=0).to(DEV)
        marks = []

        def on_step(i, lat):
            torch.cuda.synchronize()
            marks.append(time.perf_counter())

        torch.cuda.synchronize()
        marks.append(time.perf_counter())
        model.denoise(latent, ctx_c, kw["ctx_uncond"], buf, sched, kw["cfg_scale"], steps=range(n), on_step=on_step,
                      **(dict(nag=kw["nag"]) if "nag" in kw else {}))
        per = [b - a for a, b in zip(marks[:-1], marks[1:])][args.warm_steps:]
        assert bool(torch.isfinite(latent).all())
        result["arms"][name] = dict(median_s=round(statistics.median(per), 4), min_s=round(min(per), 4), max_s=round(max(per), 4))
        print(name, result["arms"][name], flush=True)
    a = result["arms"]
    result["nag_step_over_cfg5_step"] = round(a["cfg_scale=1+nag"]["median_s"] / a["cfg_scale=5"]["median_s"], 4)
    result["nag_step_over_plain_cfg1_step"] = round(a["cfg_scale=1+nag"]["median_s"] / a["cfg_scale=1"]["median_s"], 4)
    write(args.out_step, result)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
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
