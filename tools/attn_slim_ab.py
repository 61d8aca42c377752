"""What is the slim key loop of csrc/attn7p.hip worth?  attn7p_slim = 1 (steady intervals without the loop-control tests, DMA requests
from running tile pointers with one M0 write per K or V pair) against 0 (the one loop) in ONE process, both on attn_mfma = 16 and
attn_tile16_lean = 1: the two arms interleaved, the order alternating from round to round, random N(0, 1) bf16 inputs (never zeros: the kernels sit on the
power limit and the operand toggling is part of what is measured).  Every round is a timed window of at least --window seconds of
back-to-back launches; every round's number is kept and printed.  The outputs of the two arms must be EQUAL.

Shapes: the 14B self-attention (37 440 x 37 440, 40 heads) and its sequence-parallel shard shapes (9 360 and 4 680 query rows against
all keys).

The verdict a default is set by (profiles/attn_slim_loop/README.md): the slim loop wins a shape only if EVERY round of its arm is
faster than EVERY round of the one loop's.  Run on the GPU box:  python tools/attn_slim_ab.py [--out result.json]"""
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

    def set_arm(slim):
        assert ops.lib.icv_set_option(b"attn_mfma", 16 if slim >= 0 else -1) == 0
        assert ops.lib.icv_set_option(b"attn_tile16_lean", 1 if slim >= 0 else -1) == 0
        assert ops.lib.icv_set_option(b"attn7p_slim", slim) == 0

    for name in a.shapes.split(","):
        n, S = SHAPES[name]
        q = torch.randn((n, D_MODEL), device="cuda").to(torch.bfloat16)
        k = (torch.randn((S, D_MODEL), device="cuda") * (128 ** -0.5 * math.log2(math.e))).to(torch.bfloat16)
        v = torch.randn((S, D_MODEL), device="cuda").to(torch.bfloat16)
        o = {1: torch.empty_like(q), 0: torch.empty_like(q)}

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
            warm = {arm: run(arm, 3) for arm in (1, 0)}
            equal = bool(torch.equal(o[1], o[0]))
            reps = {arm: max(2, int(math.ceil(a.window * 1e3 / warm[arm]))) for arm in (1, 0)}
            ms = {1: [], 0: []}
            for r in range(a.rounds):
                for arm in ((1, 0) if r % 2 == 0 else (0, 1)):
                    ms[arm].append(run(arm, reps[arm]))
        finally:
            set_arm(-1)
        fl = 4.0 * n * S * D_MODEL
        wins = max(ms[1]) < min(ms[0])
        med = {arm: sorted(ms[arm])[len(ms[arm]) // 2] for arm in (1, 0)}
        result["shapes"][name] = {
            "q_rows": n, "keys": S, "heads": H, "launches_per_window": reps, "ms_slim": ms[1], "ms_one": ms[0],
            "median_ms": {"slim": med[1], "one": med[0]}, "tflops_median": {"slim": fl / med[1] / 1e9, "one": fl / med[0] / 1e9},
            "ratio_slim_over_one": med[1] / med[0], "every_slim_round_faster_than_every_one_round": wins, "outputs_equal": equal}
        print(f"{name:11s} {n:6d} x {S:6d} keys: slim {med[1]:8.3f} ms ({fl / med[1] / 1e9:7.1f} TF/s)  one loop {med[0]:8.3f} ms "
              f"({fl / med[0] / 1e9:7.1f} TF/s)  slim / one time {med[1] / med[0]:.4f}  ranges slim [{min(ms[1]):.3f}, {max(ms[1]):.3f}] "
              f"one loop [{min(ms[0]):.3f}, {max(ms[0]):.3f}]  slim wins every round: {wins}  outputs equal: {equal}", flush=True)
        print(f"            rounds slim    : {' '.join('%.3f' % x for x in ms[1])}", flush=True)
        print(f"            rounds one loop: {' '.join('%.3f' % x for x in ms[0])}", flush=True)
        assert equal, name + ": the two loops' outputs differ"
        del q, k, v, o
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
