"""Time per launch of the two fused latent updates that end a denoising step (run on the GPU box): icv_unpatchify_cfg_euler and
icv_unpatchify_cfg_multistep at the 14B / 480p latent (16 x 21 x 60 x 104, 32760 tokens), warm, in one process, the two kernels
alternating; each launch between its own pair of device events, the median of --launches launches reported.

    python tools/solver_update_bench.py --out profiles/solver_update_kernels.json
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from infinicube_amd.videogen import solver  # noqa: E402
from infinicube_amd.videogen.ops import HipOps  # noqa: E402
from infinicube_amd.videogen.scheduler import flow_match_sigmas  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda:0"
    ops = HipOps(dev)
    shape = (16, 21, 60, 104)
    n_tok = 21 * 30 * 52
    g = torch.Generator().manual_seed(0)
    heads = torch.randn((2, n_tok, 64), generator=g).to(dev)
    lat_e, lat_m = torch.randn(shape, generator=g).to(dev), torch.randn(shape, generator=g).to(dev)
    x_hat, ring = torch.randn(shape, generator=g).to(dev), [torch.randn(shape, generator=g).to(dev) for _ in range(3)]
    st = solver.MultistepPlan("unipc", flow_match_sigmas(25)).steps()[12]          # a mid-loop step: both orders 2, every buffer read
    assert st.order == 2 and st.corrector_order == 2

    def euler(k):
        ops.unpatchify_cfg_euler(lat_e, heads[0], heads[1], 5.0, -1e-3, 0, n_tok)

    def multistep(k):
        ops.unpatchify_cfg_multistep(lat_m, x_hat, ring[k % 3], ring[(k - 1) % 3], ring[(k - 2) % 3], heads[0], heads[1], 5.0,
                                     st.sigma, st.a, st.c, 0, n_tok)

    times = {"icv_unpatchify_cfg_euler": [], "icv_unpatchify_cfg_multistep": []}
    for k in range(args.warmup + args.launches):
        for name, fn in (("icv_unpatchify_cfg_euler", euler), ("icv_unpatchify_cfg_multistep", multistep)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(k)
            e1.record()
            torch.cuda.synchronize()
            if k >= args.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
        if k % 3 == 2:                                                            # keep the iterates finite over many launches
            lat_m.normal_(generator=None)
    elems = 16 * 21 * 60 * 104
    # bytes the algorithm needs: both head outputs read once; latent read + written; the multistep update also reads x_hat and two
    # x0-predictions and writes x_hat and one x0-prediction
    need = {"icv_unpatchify_cfg_euler": (2 + 2) * elems * 4, "icv_unpatchify_cfg_multistep": (2 + 2 + 3 + 2) * elems * 4}
    result = dict(what="time per launch of the fused latent update, one pair of device events per launch, warm, kernels alternating in one process",
                  latent=list(shape), tokens=n_tok, launches=args.launches, warmup=args.warmup, device=torch.cuda.get_device_name(0),
                  step=dict(order=st.order, corrector_order=st.corrector_order), kernels={})
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
