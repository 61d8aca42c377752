"""What is the staggered long-key kernel of csrc/attn7p.hip worth?  attn7p_stagger = 1 (att7p::attn7ps_kernel: the two waves of a SIMD in
opposite phases of the tile, a barrier per 64 keys) in its four compile-time variants - with and without the s_setprio window
(attn7p_stagger_setprio = 1 / 0), waves 0-3 or waves 4-7 opening a slot with the softmax (attn7p_stagger_swap = 1 / 0) - against
attn7p_stagger = 0 (the slim loop) in ONE process, all on attn_mfma = 16, attn_tile16_lean = 1 and attn7p_slim = 1: the arms
interleaved, their order reversed from round to round, random N(0, 1) bf16 inputs (never zeros: the kernels sit on the power limit and
the operand toggling is part of what is measured).  Every round is a timed window of at least --window seconds of back-to-back
launches; every round's number is kept and printed.  The outputs of all arms must be EQUAL on the full-size operands.

Shapes: the 14B self-attention (37 440 x 37 440, 40 heads) and its sequence-parallel shard shapes (9 360 and 4 680 query rows against
all keys).

The verdict a default is set by (profiles/attn_stagger/README.md): a staggered arm wins a shape only if EVERY round of it is faster
than EVERY round of the slim loop's.  Run on the GPU box:  python tools/attn_stagger_ab.py [--out result.json]"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from infinicube_amd.videogen.ops import HipOps  # noqa: E402

SHAPES = {"self_14b": (37440, 37440), "shard_9360": (9360, 37440), "shard_4680": (4680, 37440)}
H, D_MODEL = 40, 5120
SCALE = math.log(2.0)          # unit scale: the softmax scale and log2 e are folded into K, as the DiT does
# arm: (attn7p_stagger, attn7p_stagger_setprio, attn7p_stagger_swap); swap = 1: waves 0-3 open a slot with the softmax, waves 4-7 with QK^T
ALL_ARMS = {"slim": (0, -1, -1), "swap_setprio": (1, 1, 1), "swap_no_setprio": (1, 0, 1), "setprio": (1, 1, 0), "no_setprio": (1, 0, 0)}
ARMS = {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--window", type=float, default=0.45, help="seconds of launches per timed window (>= 0.45)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--arms", default=",".join(ALL_ARMS), help="slim and the staggered variants to set against it")
    a = ap.parse_args()
    ARMS.update({n: ALL_ARMS[n] for n in a.arms.split(",")})
    assert a.rounds >= 9 and a.window >= 0.45
    ops = HipOps("cuda:0")
    torch.manual_seed(0)
    result = {"rounds": a.rounds, "window_s": a.window, "shapes": {}}

    def set_arm(arm):
        stagger, prio, swap = ARMS[arm] if arm else (-1, -1, -1)
        for name, value in (("attn_mfma", 16 if arm else -1), ("attn_tile16_lean", 1 if arm else -1), ("attn7p_slim", 1 if arm else -1),
                            ("attn7p_stagger", stagger), ("attn7p_stagger_setprio", prio), ("attn7p_stagger_swap", swap)):
            assert ops.lib.icv_set_option(name.encode(), value) == 0

    for name in a.shapes.split(","):
        n, S = SHAPES[name]
        q = torch.randn((n, D_MODEL), device="cuda").to(torch.bfloat16)
        k = (torch.randn((S, D_MODEL), device="cuda") * (128 ** -0.5 * math.log2(math.e))).to(torch.bfloat16)
        v = torch.randn((S, D_MODEL), device="cuda").to(torch.bfloat16)
        o = {arm: torch.empty_like(q) for arm in ARMS}

        def run(arm, reps):
            set_arm(arm)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                ops.attention(q, k, v, o[arm], H, SCALE)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / reps

        try:
            warm = {arm: run(arm, 3) for arm in ARMS}
            equal = all(bool(torch.equal(o["slim"], o[arm])) for arm in ARMS)
            reps = {arm: max(2, int(math.ceil(a.window * 1e3 / warm[arm]))) for arm in ARMS}
            ms = {arm: [] for arm in ARMS}
            for r in range(a.rounds):
                for arm in (list(ARMS) if r % 2 == 0 else list(ARMS)[::-1]):
                    ms[arm].append(run(arm, reps[arm]))
        finally:
            set_arm(None)
        fl = 4.0 * n * S * D_MODEL
        med = {arm: sorted(ms[arm])[len(ms[arm]) // 2] for arm in ARMS}
        wins = {arm: max(ms[arm]) < min(ms["slim"]) for arm in ARMS if arm != "slim"}
        result["shapes"][name] = {"q_rows": n, "keys": S, "heads": H, "launches_per_window": reps, "ms": ms, "median_ms": med,
                                  "tflops_median": {arm: fl / med[arm] / 1e9 for arm in ARMS},
                                  "ratio_over_slim": {arm: med[arm] / med["slim"] for arm in ARMS},
                                  "every_round_faster_than_every_slim_round": wins, "outputs_equal": equal}
        for arm in ARMS:
            print(f"{name:11s} {n:6d} x {S:6d} keys  {arm:18s} median {med[arm]:8.3f} ms ({fl / med[arm] / 1e9:7.1f} TF/s)  / slim {med[arm] / med['slim']:.4f}  "
                  f"range [{min(ms[arm]):.3f}, {max(ms[arm]):.3f}]" + (f"  wins every round: {wins[arm]}" if arm in wins else "") +
                  f"  rounds: {' '.join('%.3f' % x for x in ms[arm])}", flush=True)
        print(f"{name:11s} outputs equal: {equal}", flush=True)
        assert equal, name + ": the arms' outputs differ"
        del q, k, v, o
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
