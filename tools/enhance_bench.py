"""What Enhance-A-Video costs (run on the GPU box), in two parts.

Kernels (--out-kernels): icv_enhance_scores_bf16 and icv_enhance_apply_bf16 at 37 440 x 5120 (T = 24, P = 1560, 40 heads) and
32 760 x 1536 (T = 21, P = 1560, 12 heads), next to icv_rmsnorm_rope on the same q, k from the same process - a kernel that reads AND
writes the bytes the score kernel only reads, i.e. a 2x traffic margin for the score kernel's strided 256-byte gather.  Warm, the
kernels alternating, each launch between its own pair of device events, the median of --launches launches.

Steps (--out-step): at synthetic weights of --model, 93 frames 480 x 832, bf16, after --warm-steps steps the median of --steps steps of
(a) cfg_scale = 5 as it is, (b) the same with enhance_weight.  With --plain-only only (a) runs and nothing of the feature is touched:
that is how the parent commit's plain step is timed from its own checkout in the same session (--parent-step adds its file to the
result).

    python tools/enhance_bench.py --out-kernels profiles/enhance_kernels.json --out-step profiles/enhance_step.json
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
from infinicube_amd.videogen.ops import HipOps, RopeTable  # noqa: E402
from infinicube_amd.videogen.scheduler import FlowMatchScheduler  # noqa: E402

DEV = "cuda:0"
WEIGHT = 4.0
LN2 = 0.6931471805599453


def write(path, result):
    print(json.dumps(result), flush=True)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


def kernels(ops, args):
    result = dict(what="time per launch, one pair of device events per launch, warm, the kernels alternating in one process; q and k are "
                       "normal draws (k at the engine's folded scale); bytes: scores reads q and k once (4 per element of one plane), "
                       "rmsnorm_rope reads and writes both (8), apply reads and writes att (4)",
                  launches=args.launches, warmup=args.warmup, device=torch.cuda.get_device_name(0), weight=WEIGHT, shapes=[])
    for T, P, H in ((24, 1560, 40), (21, 1560, 12)):
        rows, d = T * P, H * 128
        grid = TokenGrid(4 * (T - 1) + 1, 480, 832)
        assert grid.T == T and grid.tokens_per_frame == P
        g = torch.Generator().manual_seed(rows)
        q = torch.randn((rows, d), generator=g).to(torch.bfloat16).to(DEV)
        k = (torch.randn((rows, d), generator=g) * (1.4426950408889634 / 128 ** 0.5)).to(torch.bfloat16).to(DEV)
        q0, k0 = q.clone(), k.clone()
        att = torch.randn((rows, d), generator=g).to(torch.bfloat16).to(DEV)
        wq, wk = torch.ones(d, device=DEV), torch.ones(d, device=DEV)
        rope = RopeTable.build(grid.T, grid.Hp, grid.Wp, DEV, 128)                 # as the engine calls it: both norms, both rotations
        ws = torch.zeros((P,), device=DEV)
        out = torch.zeros((1,), device=DEV)
        fns = {"icv_enhance_scores_bf16": lambda: ops.enhance_scores(q, k, T, P, H, LN2, WEIGHT, ws),
               "icv_rmsnorm_rope": lambda: ops.rmsnorm_rope(q, wq, k, wk, eps=1e-6, rope=rope, tok0=0),
               "icv_enhance_apply_bf16": lambda: ops.enhance_apply(att, ws, T, P, H, WEIGHT, out)}
        times = {name: [] for name in fns}
        for it in range(args.warmup + args.launches):
            q.copy_(q0); k.copy_(k0)                                                # rmsnorm_rope runs in place: every round from the same q, k
            for name, fn in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if it >= args.warmup:
                    times[name].append(e0.elapsed_time(e1) * 1e3)
        per_element = {"icv_enhance_scores_bf16": 4, "icv_rmsnorm_rope": 8, "icv_enhance_apply_bf16": 4}
        row = dict(frames=T, positions=P, heads=H, rows=rows, d=d, E=round(float(out), 6), kernels={})
        for name, t in times.items():
            med = statistics.median(t)
            row["kernels"][name] = dict(median_us=round(med, 2), min_us=round(min(t), 2), max_us=round(max(t), 2),
                                        gb_per_s_at_median=round(per_element[name] * rows * d / med / 1e3, 1))
        kk = row["kernels"]
        row["scores_over_rmsnorm_rope_time"] = round(kk["icv_enhance_scores_bf16"]["median_us"] / kk["icv_rmsnorm_rope"]["median_us"], 3)
        result["shapes"].append(row)
        del q, k, q0, k0, att
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
    arms = [("cfg_scale=5", {})]
    if not args.plain_only:
        from infinicube_amd.videogen.enhance import EnhancePlan
        arms.append(("cfg_scale=5+enhance", dict(enhance=EnhancePlan(WEIGHT))))
    result = dict(what=f"seconds per denoising step, median of {args.steps} after {args.warm_steps} warm steps, host clock around a synchronised step",
                  model=args.model, frames=args.frames, height=args.height, width=args.width, tokens=grid.S, layers=cfg.num_layers, dtype="bf16",
                  data="synthetic weights and inputs", device=torch.cuda.get_device_name(0), weight=WEIGHT, arms={})
    for name, kw in arms:
        latent = syn.make_latent_noise(grid, seed=0).to(DEV)
        marks = []

        def on_step(i, lat):
            torch.cuda.synchronize()
            marks.append(time.perf_counter())

        torch.cuda.synchronize()
        marks.append(time.perf_counter())
        model.denoise(latent, ctx_c, ctx_u, buf, sched, 5.0, steps=range(n), on_step=on_step, **kw)
        per = [b - a for a, b in zip(marks[:-1], marks[1:])][args.warm_steps:]
        assert bool(torch.isfinite(latent).all())
        result["arms"][name] = dict(median_s=round(statistics.median(per), 4), min_s=round(min(per), 4), max_s=round(max(per), 4))
        if "enhance" in kw:
            result["arms"][name]["E_last_forward"] = model.enhance_scores
        print(name, result["arms"][name], flush=True)
    a = result["arms"]
    if args.parent_step:
        with open(args.parent_step) as f:
            a["parent commit, cfg_scale=5"] = json.load(f)["arms"]["cfg_scale=5"]
    if "cfg_scale=5+enhance" in a:
        result["enhance_step_over_plain_step"] = round(a["cfg_scale=5+enhance"]["median_s"] / a["cfg_scale=5"]["median_s"], 4)
        if args.parent_step:
            base = a["parent commit, cfg_scale=5"]["median_s"]
            result["enhance_step_over_parent_plain_step"] = round(a["cfg_scale=5+enhance"]["median_s"] / base, 4)
            result["plain_step_over_parent_plain_step"] = round(a["cfg_scale=5"]["median_s"] / base, 4)
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
    ap.add_argument("--plain-only", action="store_true", help="time the plain step only; touches nothing of the feature (a parent checkout)")
    ap.add_argument("--parent-step", default=None, help="the --out-step file of a --plain-only run from the parent commit's checkout")
    args = ap.parse_args()
    ops = HipOps(DEV)
    if not args.skip_kernels:
        kernels(ops, args)
    if not args.skip_step:
        steps(ops, args)


if __name__ == "__main__":
    main()
