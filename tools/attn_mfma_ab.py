"""What is the MFMA shape worth inside the bf16 attention kernels?  attn_mfma = 16 (v_mfma_f32_16x16x32_bf16) against 32
(v_mfma_f32_32x32x16_bf16) at the same wave tile, ring and softmax (csrc/attn_common.h: attc::tile16), in ONE process: the two arms
interleaved, the order alternating from round to round, random N(0, 1) bf16 inputs (never zeros: both shapes tie on zeros, the
kernels sit on the power limit and the operand toggling is part of what is measured).  Every round is a timed window of at least
--window seconds of back-to-back launches; every round's number is kept and printed.

Shapes: the 14B self-attention (37 440 x 37 440, 40 heads), its sequence-parallel shard shapes (9 360 and 4 680 query rows against
all keys) and the 512-key cross-attention (attn7.hip's short-key kernel).

The verdict the default is set by (profiles/attn_mfma16/README.md): 16 wins a shape only if EVERY round of the 16 arm is faster
than EVERY round of the 32 arm.  Run on the GPU box:  python tools/attn_mfma_ab.py [--out result.json]"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from infinicube_amd.videogen.ops import HipOps  # noqa: E402

SHAPES = {"self_14b": (37440, 37440), "shard_9360": (9360, 37440), "shard_4680": (4680, 37440), "cross_512": (37440, 512)}
H, D_MODEL = 40, 5120
SCALE = math.log(2.0)          # unit scale: the softmax scale and log2 e are folded into K, as the DiT does


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--window", type=float, default=0.45, help="seconds of launches per timed window (>= 0.4)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.rounds >= 9 and a.window >= 0.4
    ops = HipOps("cuda:0")
    torch.manual_seed(0)
    result = {"rounds": a.rounds, "window_s": a.window, "shapes": {}}

    def set_mf(mf):
        assert ops.lib.icv_set_option(b"attn_mfma", mf) == 0

    for name in a.shapes.split(","):
        n, S = SHAPES[name]
        q = torch.randn((n, D_MODEL), device="cuda").to(torch.bfloat16)
        k = (torch.randn((S, D_MODEL), device="cuda") * (128 ** -0.5 * math.log2(math.e))).to(torch.bfloat16)
        v = torch.randn((S, D_MODEL), device="cuda").to(torch.bfloat16)
        o = {16: torch.empty_like(q), 32: torch.empty_like(q)}

        def run(mf, reps):
            set_mf(mf)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                ops.attention(q, k, v, o[mf], H, SCALE)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / reps

        try:
            warm = {mf: run(mf, 3) for mf in (16, 32)}
            diff = (o[16].float() - o[32].float())
            rms = float(o[32].float().pow(2).mean().sqrt())
            reps = {mf: max(2, int(math.ceil(a.window * 1e3 / warm[mf]))) for mf in (16, 32)}
            ms = {16: [], 32: []}
            for r in range(a.rounds):
                for mf in ((16, 32) if r % 2 == 0 else (32, 16)):
                    ms[mf].append(run(mf, reps[mf]))
        finally:
            set_mf(-1)
        fl = 4.0 * n * S * D_MODEL
        wins = max(ms[16]) < min(ms[32])
        med = {mf: sorted(ms[mf])[len(ms[mf]) // 2] for mf in (16, 32)}
        result["shapes"][name] = {
            "q_rows": n, "keys": S, "heads": H, "launches_per_window": reps, "ms_16": ms[16], "ms_32": ms[32],
            "median_ms": med, "tflops_median": {mf: fl / med[mf] / 1e9 for mf in (16, 32)}, "ratio_16_over_32": med[16] / med[32],
            "every_16_round_faster_than_every_32_round": wins,
            "out_rms_diff_over_rms": float(diff.pow(2).mean().sqrt()) / rms, "out_max_abs_diff": float(diff.abs().max())}
        print(f"{name:11s} {n:6d} x {S:6d} keys: 16x16x32 {med[16]:8.3f} ms ({fl / med[16] / 1e9:7.1f} TF/s)  32x32x16 {med[32]:8.3f} ms "
              f"({fl / med[32] / 1e9:7.1f} TF/s)  16 / 32 time {med[16] / med[32]:.4f}  ranges 16 [{min(ms[16]):.3f}, {max(ms[16]):.3f}] "
              f"32 [{min(ms[32]):.3f}, {max(ms[32]):.3f}]  16 wins every round: {wins}", flush=True)
        print(f"            rounds 16: {' '.join('%.3f' % x for x in ms[16])}", flush=True)
        print(f"            rounds 32: {' '.join('%.3f' % x for x in ms[32])}", flush=True)
        del q, k, v, o
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
