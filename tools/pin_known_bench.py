"""Time per launch of the two input_mask kernels (run on the GPU box): icv_pin_known_f32 at the 14B / 480p latent (16 x 21 x 60 x 104)
with 3 of 21 latent frames kept and with all kept, each Euler-only (the latent) and with the multistep solver's state (x_hat + m_new),
next to icv_add_noise_f32 and icv_unpatchify_cfg_euler at the same shape, and icv_latent_keep_mask_u8 at 81 x 480 x 832 - warm, in one
process, the kernels alternating; each launch between its own pair of device events, the median of --launches launches reported.

    python tools/pin_known_bench.py --out profiles/pin_known_kernels.json
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

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
    x0, noise, lat, x_hat, m_new, out = (torch.randn(shape, generator=g).to(dev) for _ in range(6))
    heads = torch.randn((2, n_tok, cols), generator=g).to(dev)
    keeps = {"3_of_21": torch.zeros(shape[1:], dtype=torch.uint8), "all": torch.ones(shape[1:], dtype=torch.uint8)}
    keeps["3_of_21"][:3] = 1
    keeps = {k: v.to(dev) for k, v in keeps.items()}
    mask = torch.ones((81, 480, 832), dtype=torch.uint8)
    mask[:9] = 0
    mask = mask.to(dev)
    keep_out = torch.empty(shape[1:], dtype=torch.uint8, device=dev)
    elems, cells = lat.numel(), keeps["all"].numel()

    def pin(keep, state):
        return lambda: ops.pin_known(lat, x0, noise, keeps[keep], 0.5, x_hat=x_hat if state else None, sigma_cur=0.6,
                                     m_new=m_new if state else None)

    # name -> (launch, bytes the algorithm needs).  The pin reads every keep byte once per channel, and x0 + noise of the kept
    # elements; it writes the latent (and x_hat and m_new) there.
    kernels = {}
    for keep, frac in (("3_of_21", 3 / 21), ("all", 1.0)):
        kept = int(elems * frac) * 4
        kernels[f"icv_pin_known_f32[{keep},euler]"] = (pin(keep, False), 16 * cells + 3 * kept)
        kernels[f"icv_pin_known_f32[{keep},x_hat+m_new]"] = (pin(keep, True), 16 * cells + 5 * kept)
    kernels["icv_add_noise_f32"] = (lambda: ops.add_noise(x0, noise, out, 0.5), 3 * elems * 4)
    kernels["icv_unpatchify_cfg_euler"] = (lambda: ops.unpatchify_cfg_euler(lat, heads[0], heads[1], 5.0, -1e-3, 0, n_tok), 4 * elems * 4)
    kernels["icv_latent_keep_mask_u8"] = (lambda: ops.latent_keep_mask(mask, keep_out), mask.numel() + cells)

    times = {name: [] for name in kernels}
    for k in range(args.warmup + args.launches):
        for name, (fn, _) in kernels.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if k >= args.warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    assert int(keep_out.sum()) == 3 * 60 * 104                         # 9 frames kept = latent frames 0, 1, 2
    result = dict(what="time per launch, one pair of device events per launch, warm, the kernels alternating in one process",
                  latent=list(shape), mask=list(mask.shape), launches=args.launches, warmup=args.warmup,
                  device=torch.cuda.get_device_name(0), kernels={})
    for name, t in times.items():
        med = statistics.median(t)
        result["kernels"][name] = dict(median_us=round(med, 2), min_us=round(min(t), 2), max_us=round(max(t), 2),
                                       bytes_needed=kernels[name][1], gb_per_s_at_median=round(kernels[name][1] / med / 1e3, 1))
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
