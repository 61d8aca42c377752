"""What EasyCache costs and saves (run on the GPU box), in two parts.

Kernels (--out-kernels): icv_l1_change_f64 (the latent as one row, with and without the in-pass copy; the conditional head output with
the copy) and icv_easycache_predict_f32 (both branches) at the 14B / 480p shapes - latent 16 x 21 x 60 x 104, head outputs
32 760 x 64 - next to icv_unpatchify_cfg_euler on the same buffers from the same process.  Warm, the kernels alternating, each call
between its own pair of device events (icv_l1_change_f64 is two launches: both are inside), the median of --launches calls.

Steps (--out-step): at synthetic weights of --model, 93 frames 480 x 832, bf16, cfg_scale = 5, after --warm-steps steps the median of
--steps steps of (a) the plain loop, (b) the loop with the cache on and a threshold nothing stays under, where the plan's force_skip
makes every second step after the warm ones a skipped one: --steps computed and --steps skipped steps, timed apart.  The two loops
alternate --rounds times in the one process (off, on, off, on); per-round figures and the pooled medians are written.  With
--plain-only only (a) runs and nothing of the feature is touched: that is how the parent commit's plain step is timed from its own
checkout in the same session (--parent-step adds its file to the result).

    python tools/easy_cache_bench.py --out-kernels profiles/easy_cache_kernels.json --out-step profiles/easy_cache_step.json
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
    from infinicube_amd import native
    grid = TokenGrid(81, 480, 832)                      # 21 latent frames of 30 x 52 tokens
    C, (T, H8, W8) = 16, grid.latent_shape()[1:]
    assert (T, H8, W8, grid.S) == (21, 60, 104, 32760)
    n_tok, cols = grid.S, 4 * C
    g = torch.Generator().manual_seed(1)
    x, x_b = (torch.randn((C, T, H8, W8), generator=g).to(DEV) for _ in range(2))
    hc, hu, hcl, hul = (torch.randn((n_tok, cols), generator=g).to(DEV) for _ in range(4))
    work = torch.zeros((native.L1_CHANGE_WORKSPACE_DOUBLES,), dtype=torch.float64, device=DEV)
    sums = torch.zeros((8,), dtype=torch.float64, device=DEV)
    lat = x.clone()
    fns = {"icv_l1_change_f64 latent": lambda: ops.l1_change(x.view(1, -1), x_b.view(1, -1), work, sums[0:2]),
           "icv_l1_change_f64 latent, update_b": lambda: ops.l1_change(x.view(1, -1), x_b.view(1, -1), work, sums[2:4], update_b=True),
           "icv_l1_change_f64 head, update_b": lambda: ops.l1_change(hc, hcl, work, sums[4:6], update_b=True),
           "icv_easycache_predict_f32 two branches": lambda: ops.easycache_predict(x, x_b, hcl, hul, hc, hu, 0, n_tok),
           "icv_unpatchify_cfg_euler": lambda: ops.unpatchify_cfg_euler(lat, hc, hu, 5.0, -1e-3, 0, n_tok)}
    # bytes moved per call: l1 reads a and b (update: writes b); predict reads 2 latents + 2 heads, writes 2 heads; euler reads 2 heads, reads + writes the latent
    nl, nh = x.numel() * 4, n_tok * cols * 4
    moved = {"icv_l1_change_f64 latent": 2 * nl, "icv_l1_change_f64 latent, update_b": 3 * nl, "icv_l1_change_f64 head, update_b": 3 * nh,
             "icv_easycache_predict_f32 two branches": 2 * nl + 4 * nh, "icv_unpatchify_cfg_euler": 2 * nh + 2 * nl}
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
    # the blocking read of one step's sums, host clock, the stream idle
    reads = []
    for it in range(args.warmup + args.launches):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.read_doubles(sums)
        if it >= args.warmup:
            reads.append((time.perf_counter() - t0) * 1e6)
    result = dict(what="time per call, one pair of device events per call, warm, the kernels alternating in one process; normal draws; "
                       "icv_l1_change_f64 is two launches per call; read_doubles: host clock around the 64-byte blocking read on an idle stream",
                  launches=args.launches, warmup=args.warmup, device=torch.cuda.get_device_name(0), latent=[C, T, H8, W8], heads=[n_tok, cols],
                  kernels={}, read_doubles_us=dict(median=round(statistics.median(reads), 2), min=round(min(reads), 2), max=round(max(reads), 2)))
    for name, t in times.items():
        med = statistics.median(t)
        result["kernels"][name] = dict(median_us=round(med, 2), min_us=round(min(t), 2), max_us=round(max(t), 2), bytes=moved[name],
                                       gb_per_s_at_median=round(moved[name] / med / 1e3, 1))
    assert bool(torch.isfinite(sums[:6]).all())
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
    result = dict(what=f"seconds per denoising step, median of {args.steps} after {args.warm_steps} warm steps, host clock around a synchronised step",
                  model=args.model, frames=args.frames, height=args.height, width=args.width, tokens=grid.S, layers=cfg.num_layers, dtype="bf16",
                  data="synthetic weights and inputs", device=torch.cuda.get_device_name(0), arms={})

    def run(n, **kw):
        latent = syn.make_latent_noise(grid, seed=0).to(DEV)
        marks = []

        def on_step(i, lat):
            torch.cuda.synchronize()
            marks.append(time.perf_counter())

        torch.cuda.synchronize()
        marks.append(time.perf_counter())
        model.denoise(latent, ctx_c, ctx_u, buf, sched, 5.0, steps=range(n), on_step=on_step, **kw)
        assert bool(torch.isfinite(latent).all())
        return [b - a for a, b in zip(marks[:-1], marks[1:])]

    def arm(name, per):
        result["arms"][name] = dict(median_s=round(statistics.median(per), 4), min_s=round(min(per), 4), max_s=round(max(per), 4), steps=len(per))
        print(name, result["arms"][name], flush=True)

    # the arms alternate in this one process: off, on, off, on ...; every loop starts with its own warm steps
    off, on_computed, on_skipped = [], [], []
    for r in range(args.rounds):
        off.append(run(args.warm_steps + args.steps)[args.warm_steps:])
        arm(f"cache off, round {r + 1}", off[-1])
        if args.plain_only:
            continue
        from infinicube_amd.videogen.easycache import EasyCachePlan
        w, n = args.warm_steps, args.warm_steps + 2 * args.steps
        skip = frozenset(range(w + 1, n, 2))
        plan = EasyCachePlan(1e-12, max(w, 2), skip)
        per = run(n, easy_cache=plan)
        rec = plan.record()
        assert rec["skipped"] == sorted(skip), rec
        on_computed.append([per[i] for i in rec["computed"] if i >= w])
        on_skipped.append([per[i] for i in rec["skipped"]])
        arm(f"cache on, computed step, round {r + 1}", on_computed[-1])
        arm(f"cache on, skipped step, round {r + 1}", on_skipped[-1])
        result["record"] = rec
    arm("cache off", sum(off, []))
    if on_computed:
        arm("cache on, computed step", sum(on_computed, []))
        arm("cache on, skipped step", sum(on_skipped, []))
    a = result["arms"]
    if args.parent_step:
        with open(args.parent_step) as f:
            a["parent commit, plain step"] = json.load(f)["arms"]["cache off"]
    if "cache on, computed step" in a:
        off = a["cache off"]["median_s"]
        result["computed_step_over_cache_off_step"] = round(a["cache on, computed step"]["median_s"] / off, 4)
        result["skipped_step_over_cache_off_step"] = round(a["cache on, skipped step"]["median_s"] / off, 5)
        if args.parent_step:
            base = a["parent commit, plain step"]["median_s"]
            result["cache_off_step_over_parent_plain_step"] = round(off / base, 4)
            result["computed_step_over_parent_plain_step"] = round(a["cache on, computed step"]["median_s"] / base, 4)
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
    ap.add_argument("--rounds", type=int, default=2, help="how often the step arms alternate (off, on, off, on ...)")
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
