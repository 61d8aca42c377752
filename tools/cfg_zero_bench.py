"""Time per call of the CFG-Zero* optimised scale (run on the GPU box): icv_cfg_zero_scale_f32 - both of its launches - at the
14B / 480p head shape (32760 tokens x 64 columns), next to icv_unpatchify_cfg_euler at the same latent (16 x 21 x 60 x 104), warm, in
one process, the two alternating; each call between its own pair of device events, the median of --launches calls reported.

    python tools/cfg_zero_bench.py --out profiles/cfg_zero_kernels.json
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from infinicube_amd import native  # noqa: E402
from infinicube_amd.videogen.ops import HipOps  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda:0"
    ops = HipOps(dev)
    shape = (16, 21, 60, 104)
    n_tok, cols = 21 * 30 * 52, 64
    g = torch.Generator().manual_seed(0)
    u0 = torch.randn((n_tok, cols), generator=g)
    heads = torch.stack([0.7 * u0 + 0.5 * torch.randn((n_tok, cols), generator=g), u0]).to(dev)
    keep = heads[1].clone()
    lat = torch.randn(shape, generator=g).to(dev)
    work = torch.zeros(native.CFG_ZERO_WORKSPACE_DOUBLES, dtype=torch.float64, device=dev)
    scale = torch.zeros(1, device=dev)

    def zero_scale():
        ops.cfg_zero_scale(heads[0], heads[1], n_tok, work, scale)

    def euler():
        ops.unpatchify_cfg_euler(lat, heads[0], heads[1], 5.0, -1e-3, 0, n_tok)

    times = {"icv_cfg_zero_scale_f32": [], "icv_unpatchify_cfg_euler": []}
    for k in range(args.warmup + args.launches):
        heads[1].copy_(keep)                                                      # the op scales hu in place: start every call from u
        for name, fn in (("icv_cfg_zero_scale_f32", zero_scale), ("icv_unpatchify_cfg_euler", euler)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if k >= args.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    head_bytes = n_tok * cols * 4
    elems = 16 * 21 * 60 * 104
    # bytes the algorithm needs: the moments read both head outputs, the apply reads and writes one; the Euler update reads both
    # head outputs and reads + writes the latent
    need = {"icv_cfg_zero_scale_f32": 4 * head_bytes, "icv_unpatchify_cfg_euler": (2 + 2) * elems * 4}
    result = dict(what="time per call (icv_cfg_zero_scale_f32: its two launches together), one pair of device events per call, warm, the two alternating in one process",
                  head_rows=n_tok, head_cols=cols, latent=list(shape), launches=args.launches, warmup=args.warmup,
                  device=torch.cuda.get_device_name(0), scale=float(scale.cpu()), kernels={})
    for name, t in times.items():
        med = statistics.median(t)
        result["kernels"][name] = dict(median_us=round(med, 2), min_us=round(min(t), 2), max_us=round(max(t), 2),
                                       bytes_needed=need[name], gb_per_s_at_median=round(need[name] / med / 1e3, 1))
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
