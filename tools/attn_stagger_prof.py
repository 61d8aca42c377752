"""Profile the 14B self-attention launch (37 440 x 37 440, 40 heads, random N(0, 1) bf16, unit scale: the operands of
tools/attn_slim_prof.py) under rocprofv3 with attn7p_stagger = 0 (the slim loop: both waves of a SIMD in the same phase of the tile)
and = 1 (the staggered kernel of csrc/attn7p.hip), both on attn_mfma = 16, attn_tile16_lean = 1 and attn7p_slim = 1.  Per arm one
--kernel-trace --stats pass and two counter passes of their own (--pmc only, no tracing option beside it), every pass in a fresh
child process.  What the passes are for:
  * pmc_clock:  effective clock = GRBM_GUI_ACTIVE / 8 XCDs / kernel duration, MFMA busy = SQ_VALU_MFMA_BUSY_CYCLES / (1024 SIMDs x
                those cycles) - the columns of profiles/attn_slim_loop/;
  * pmc_coexec: SQ_VALU_MFMA_COEXEC_CYCLES / SQ_VALU_MFMA_BUSY_CYCLES = the share of the matrix pipe's busy cycles in which another
                VALU instruction executes beside it - what the stagger is meant to raise - and SQ_WAIT_ANY / SQ_WAVE_CYCLES.
Both arms are profiled the same way; never set a profiled number against an unprofiled one.  A library without the option (an older
commit's, through ICV_LIB_PATH) ignores it: --arms 0 profiles that library's default kernel.

    python tools/attn_stagger_prof.py --out DIR [--arms 0,1]     (drives the passes, writes DIR/summary.{json,md})
    python tools/attn_stagger_prof.py --launch 1|0               (what runs under the profiler)"""
import argparse
import json
import math
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from attn_slim_prof import D_MODEL, H, ROOT, S, rows_of  # noqa: E402

PASSES = {"stats": ["--kernel-trace", "--stats"],
          "pmc_clock": ["--pmc", "GRBM_GUI_ACTIVE", "SQ_VALU_MFMA_BUSY_CYCLES", "SQ_WAVE_CYCLES"],
          "pmc_coexec": ["--pmc", "SQ_VALU_MFMA_COEXEC_CYCLES", "SQ_VALU_MFMA_BUSY_CYCLES", "SQ_WAVE_CYCLES", "SQ_WAIT_ANY"]}
COLUMNS = [("stats_avg_us", "--stats us / launch", "%.1f"), ("effective_clock_ghz", "eff. clock GHz", "%.3f"), ("mfma_busy", "MFMA busy", "%.3f"),
           ("busy_x_clock", "busy x clock", "%.3f"), ("coexec_share", "VALU co-executing / MFMA busy", "%.3f"),
           ("wait_any_share", "SQ_WAIT_ANY / SQ_WAVE_CYCLES", "%.3f"), ("SQ_VALU_MFMA_COEXEC_CYCLES", "COEXEC cycles", "%.4g"),
           ("coexec_busy_cycles", "MFMA busy cycles", "%.4g"), ("coexec_wave_cycles", "wave cycles", "%.4g"), ("SQ_WAIT_ANY", "wait-any cycles", "%.4g")]


def launch(stagger, reps, setprio, swap):
    sys.path.insert(0, ROOT)
    import torch
    from infinicube_amd.videogen.ops import HipOps
    ops = HipOps("cuda:0")
    torch.manual_seed(0)
    q = torch.randn((S, D_MODEL), device="cuda").to(torch.bfloat16)
    k = (torch.randn((S, D_MODEL), device="cuda") * (128 ** -0.5 * math.log2(math.e))).to(torch.bfloat16)
    v = torch.randn((S, D_MODEL), device="cuda").to(torch.bfloat16)
    o = torch.empty_like(q)
    for name, value in (("attn_mfma", 16), ("attn_tile16_lean", 1), ("attn7p_slim", 1), ("attn7p_stagger", stagger),
                        ("attn7p_stagger_setprio", setprio), ("attn7p_stagger_swap", swap)):
        assert ops.lib.icv_set_option(name.encode(), value) == 0
    for _ in range(reps):
        ops.attention(q, k, v, o, H, math.log(2.0))
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launch", type=int, default=None)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--arms", default="0,1")
    ap.add_argument("--setprio", type=int, default=-1, help="attn7p_stagger_setprio of the staggered arm (negative: the default)")
    ap.add_argument("--swap", type=int, default=-1, help="attn7p_stagger_swap of the staggered arm (negative: the default)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.launch is not None:
        return launch(a.launch, a.reps, a.setprio, a.swap)
    assert a.out
    avg = lambda x: sum(x) / len(x) if x else None
    summary = {}
    for stagger in [int(x) for x in a.arms.split(",")]:
        arm, res = "stagger_%d" % stagger, {}
        for pname, flags in PASSES.items():
            d = os.path.join(a.out, arm, pname)
            os.makedirs(d, exist_ok=True)
            cmd = ["rocprofv3"] + flags + ["--output-format", "csv", "-d", d, "-o", "p", "--", sys.executable, os.path.abspath(__file__),
                   "--launch", str(stagger), "--reps", str(a.reps), "--setprio", str(a.setprio), "--swap", str(a.swap)]
            with open(os.path.join(d, "run.log"), "w") as log:
                rc = subprocess.run(cmd, stdout=log, stderr=subprocess.STDOUT, timeout=180).returncode
            if rc != 0:
                print(f"{arm} {pname}: rocprofv3 exited {rc}; stopping", flush=True)
                return rc
            tbl = rows_of(d, "*kernel_trace.csv" if pname == "stats" else "*counter_collection.csv")
            for n, v in tbl.items():
                r = res.setdefault(n, {})
                dur = v["dur"][1:] or v["dur"]            # the first launch pays the module load
                r[pname + "_avg_us"] = avg(dur)
                ctr = {c: avg(vals[1:] or vals) for c, vals in v["ctr"].items()}
                if pname == "pmc_clock" and ctr.get("GRBM_GUI_ACTIVE"):
                    r.update(ctr)
                    gui = ctr["GRBM_GUI_ACTIVE"] / 8.0
                    r["effective_clock_ghz"] = gui / ((r.get("pmc_clock_avg_us") or r["stats_avg_us"]) * 1e3)
                    r["mfma_busy"] = ctr["SQ_VALU_MFMA_BUSY_CYCLES"] / (1024.0 * gui)
                    r["busy_x_clock"] = r["mfma_busy"] * r["effective_clock_ghz"]
                if pname == "pmc_coexec" and ctr.get("SQ_VALU_MFMA_BUSY_CYCLES"):
                    r["SQ_VALU_MFMA_COEXEC_CYCLES"], r["SQ_WAIT_ANY"] = ctr.get("SQ_VALU_MFMA_COEXEC_CYCLES"), ctr.get("SQ_WAIT_ANY")
                    r["coexec_busy_cycles"], r["coexec_wave_cycles"] = ctr["SQ_VALU_MFMA_BUSY_CYCLES"], ctr.get("SQ_WAVE_CYCLES")
                    r["coexec_share"] = ctr.get("SQ_VALU_MFMA_COEXEC_CYCLES", 0.0) / ctr["SQ_VALU_MFMA_BUSY_CYCLES"]
                    if ctr.get("SQ_WAVE_CYCLES") and ctr.get("SQ_WAIT_ANY") is not None:
                        r["wait_any_share"] = ctr["SQ_WAIT_ANY"] / ctr["SQ_WAVE_CYCLES"]
        summary[arm] = res
        print(arm, json.dumps(res), flush=True)
    json.dump(summary, open(os.path.join(a.out, "summary.json"), "w"), indent=1)
    with open(os.path.join(a.out, "summary.md"), "w") as o:
        o.write("| arm | kernel | " + " | ".join(c[1] for c in COLUMNS) + " |\n|" + "---|" * (len(COLUMNS) + 2) + "\n")
        for arm, res in summary.items():
            for n, r in res.items():
                o.write(f"| {arm} | `{n[:64]}` | " + " | ".join((fmt % r[key]) if r.get(key) is not None else "-" for key, _, fmt in COLUMNS) + " |\n")
    print(open(os.path.join(a.out, "summary.md")).read())
    return 0


if __name__ == "__main__":
    sys.exit(main())
