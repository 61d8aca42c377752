"""TeaCache on the HIP loop at a real size: what a skipped and a computed step cost, what the residual store costs, and how far a
cached loop moves the latent (random-init weights, so the schedule is FORCED: every ``--every``-th step computed, plus the ends).

    python tools/teacache_study.py [--model 14b] [--steps 50] [--every 2] [--out profiles/teacache/study_14b_480p.json]

Random weights say nothing about how many steps a trained checkpoint skips at a given threshold; the line "real_coefficients"
only shows what the 14B t2v polynomial makes of these random-init distances.  Prints one JSON object."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from infinicube_amd.videogen import synthetic as syn, teacache  # noqa: E402
from infinicube_amd.videogen.config import TokenGrid, preset  # noqa: E402
from infinicube_amd.videogen.dit import WanDiT  # noqa: E402
from infinicube_amd.videogen.ops import HipOps  # noqa: E402
from infinicube_amd.videogen.scheduler import FlowMatchScheduler  # noqa: E402
from oracle.wan_ref import psnr  # noqa: E402


def _ms(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="14b")
    ap.add_argument("--frames", type=int, default=93)        # config #3: 93 frames 480x832 (bench.py)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=832)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--every", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda:0"
    ops = HipOps(dev)
    cfg, grid = preset(args.model), TokenGrid(args.frames, args.height, args.width)
    sd = syn.make_dit_state_dict(cfg, seed=0, device=dev, dtype=torch.bfloat16)
    bsd = syn.make_buffer_embedder_state_dict(cfg, device=dev, dtype=torch.bfloat16)
    m = WanDiT(cfg, sd, ops, bsd).prepare(grid, graphs=False)
    del sd, bsd
    ck, cu = m.encode_context(syn.make_text_context(cfg, 1)), m.encode_context(syn.make_text_context(cfg, 2))
    buf = m.embed_buffers(syn.make_buffer_latents(cfg, grid))
    noise = syn.make_latent_noise(grid, seed=0).to(dev)
    sch = FlowMatchScheduler(args.steps)
    n = args.steps
    real = teacache.plan(m, sch, 0.2, "Wan2.1-T2V-14B")
    forced = set(range(0, n, args.every)) | {0, n - 1}
    plan = teacache.TeaCachePlan("forced", float("nan"), real.steps, real.distances, tuple(sorted(forced)))
    res = m._tc_residuals()
    lat = noise.clone()
    m.denoise(lat, ck, cu, buf, sch, 5.0, steps=range(1), tea_cache=plan)      # fills the residuals; warms every kernel
    ts = sch.timesteps[n // 2]
    computed_ms = _ms(lambda: m.forward_pair(lat, ck, cu, ts, buf, m.head_out, share_stem=m.share_stem), 2)
    store_ms = _ms(lambda: (m._tc_store(m.patches, m._pair.x[:m.plan.n_tok], res[0]), m._tc_store(m.patches, m._pair.x[m.plan.n_tok:], res[1])), 5)

    def skipped():
        m.forward_tokens(lat, ck, ts, res[0], m.head_out[0], num_layers=0)
        m.forward_tokens(lat, cu, ts, res[1], m.head_out[1], num_layers=0)

    skipped_ms = _ms(skipped, 5)
    loops = {}
    for name, tc in (("uncached", None), ("cached", plan)):
        lat = noise.clone()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.denoise(lat, ck, cu, buf, sch, 5.0, tea_cache=tc)
        torch.cuda.synchronize()
        loops[name] = (time.perf_counter() - t0, lat.cpu())
    out = dict(
        model=args.model, grid=[grid.num_frames, grid.height, grid.width], tokens=grid.S, steps=n,
        forced_computed=len(plan.computed), forced_every=args.every,
        computed_step_ms=round(computed_ms + store_ms, 2), computed_forward_pair_ms=round(computed_ms, 2),
        store_ms_per_step=round(store_ms, 3), skipped_step_ms=round(skipped_ms, 2),
        skipped_over_computed=round(skipped_ms / (computed_ms + store_ms), 4),
        loop_s=dict(uncached=round(loops["uncached"][0], 2), cached=round(loops["cached"][0], 2)),
        speedup=round(loops["uncached"][0] / loops["cached"][0], 3),
        latent_psnr_db_cached_vs_uncached=round(psnr(loops["cached"][1], loops["uncached"][1]), 2),
        real_coefficients=dict(model_id="Wan2.1-T2V-14B", thresh=0.2, computed=len(real.computed),
                               note="random-init weights: says nothing about a trained checkpoint"),
        distances_min_max=[round(min(real.distances[1:]), 5), round(max(real.distances[1:]), 5)],
        residual_bytes_per_branch=res[0].numel() * 4,
    )
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
