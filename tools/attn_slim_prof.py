"""Profile the 14B self-attention launch (37 440 x 37 440, 40 heads, random N(0, 1) bf16, unit scale) under both forms of attn7p.hip's
key loop (attn7p_slim = 1 and 0, both on attn_mfma = 16 and attn_tile16_lean = 1) under rocprofv3: per arm one --kernel-trace --stats
pass and two counter passes of their own (--pmc only, no tracing option beside it), every pass in a fresh child process.  From the SAME counter pass: effective
clock = GRBM_GUI_ACTIVE / 8 XCDs / kernel duration, MFMA busy = SQ_VALU_MFMA_BUSY_CYCLES / (1024 SIMDs x those cycles).  Both arms are profiled the same way; never set a profiled number
against an unprofiled one.

    python tools/attn_slim_prof.py --out DIR          (drives the passes, writes DIR/summary.{json,md})
    python tools/attn_slim_prof.py --launch 1|0       (what runs under the profiler)"""
import argparse
import collections
import csv
import glob
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, H, D_MODEL = 37440, 40, 5120
PASSES = {"stats": ["--kernel-trace", "--stats"],
          "pmc_clock": ["--pmc", "GRBM_GUI_ACTIVE", "SQ_VALU_MFMA_BUSY_CYCLES", "SQ_WAVE_CYCLES"],
          "pmc_insts": ["--pmc", "SQ_INSTS_SALU", "SQ_INSTS_VALU", "SQ_INSTS_MFMA"]}


def launch(slim, reps):
    sys.path.insert(0, ROOT)
    import torch
    from infinicube_amd.videogen.ops import HipOps
    ops = HipOps("cuda:0")
    torch.manual_seed(0)
    q = torch.randn((S, D_MODEL), device="cuda").to(torch.bfloat16)
    k = (torch.randn((S, D_MODEL), device="cuda") * (128 ** -0.5 * math.log2(math.e))).to(torch.bfloat16)
    v = torch.randn((S, D_MODEL), device="cuda").to(torch.bfloat16)
    o = torch.empty_like(q)
    assert ops.lib.icv_set_option(b"attn_mfma", 16) == 0
    assert ops.lib.icv_set_option(b"attn_tile16_lean", 1) == 0
    assert ops.lib.icv_set_option(b"attn7p_slim", slim) == 0
    for _ in range(reps):
        ops.attention(q, k, v, o, H, math.log(2.0))
    torch.cuda.synchronize()


def rows_of(d, pattern):
    out = collections.defaultdict(lambda: {"dur": [], "ctr": collections.defaultdict(list)})
    for f in glob.glob(os.path.join(d, "**", pattern), recursive=True):
        seen = set()
        for r in csv.DictReader(open(f)):
            n = r["Kernel_Name"]
            if "attn7" not in n:
                continue
            if "Counter_Name" in r:
                out[n]["ctr"][r["Counter_Name"]].append(float(r["Counter_Value"]))
                if r["Dispatch_Id"] in seen:
                    continue
                seen.add(r["Dispatch_Id"])
            if r.get("Start_Timestamp") and r.get("End_Timestamp"):
                out[n]["dur"].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launch", type=int, default=None)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.launch is not None:
        return launch(a.launch, a.reps)
    assert a.out
    arms = [("slim", 1), ("one_loop", 0)]
    avg = lambda x: sum(x) / len(x) if x else None
    summary = {}
    for arm, slim in arms:
        res = {}
        for pname, flags in PASSES.items():
            d = os.path.join(a.out, arm, pname)
            os.makedirs(d, exist_ok=True)
            cmd = ["rocprofv3"] + flags + ["--output-format", "csv", "-d", d, "-o", "p", "--", sys.executable,
                   os.path.abspath(__file__), "--launch", str(slim), "--reps", str(a.reps)]
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
                r[pname + "_launches_us"] = v["dur"]
                for c, vals in v["ctr"].items():
                    r[c] = avg(vals[1:] or vals)
                if pname == "pmc_clock" and r.get("GRBM_GUI_ACTIVE"):
                    gui = r["GRBM_GUI_ACTIVE"] / 8.0
                    r["clock_from_us"] = r.get("pmc_clock_avg_us") or r["stats_avg_us"]     # a counter pass without time stamps: the --stats pass's
                    r["effective_clock_ghz"] = gui / (r["clock_from_us"] * 1e3)
                    r["mfma_busy"] = r["SQ_VALU_MFMA_BUSY_CYCLES"] / (1024.0 * gui)
        summary[arm] = res
        print(arm, json.dumps({k: {x: y for x, y in v.items() if not x.endswith("launches_us")} for k, v in res.items()}), flush=True)
    json.dump(summary, open(os.path.join(a.out, "summary.json"), "w"), indent=1)
    fl = 4.0 * S * S * D_MODEL
    with open(os.path.join(a.out, "summary.md"), "w") as o:
        o.write("| arm | kernel | --stats us / launch | TF/s | eff. clock GHz | MFMA busy | busy x clock | wave cycles | SALU insts | VALU insts | MFMA insts |\n|---|---|---|---|---|---|---|---|---|---|---|\n")
        for arm, res in summary.items():
            for n, r in res.items():
                f = lambda key, fmt: (fmt % r[key]) if r.get(key) is not None else "-"
                prod = "%.3f" % (r["mfma_busy"] * r["effective_clock_ghz"]) if r.get("mfma_busy") else "-"
                o.write(f"| {arm} | `{n[:60]}` | {f('stats_avg_us', '%.1f')} | {'%.1f' % (fl / r['stats_avg_us'] / 1e6) if r.get('stats_avg_us') else '-'} | "
                        f"{f('effective_clock_ghz', '%.3f')} | {f('mfma_busy', '%.3f')} | {prod} | {f('SQ_WAVE_CYCLES', '%.4g')} | "
                        f"{f('SQ_INSTS_SALU', '%.4g')} | {f('SQ_INSTS_VALU', '%.4g')} | {f('SQ_INSTS_MFMA', '%.4g')} |\n")
    print(open(os.path.join(a.out, "summary.md")).read())
    return 0


if __name__ == "__main__":
    sys.exit(main())
