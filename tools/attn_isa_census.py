"""Static census of the bf16 attention kernels (csrc/attn7.hip, csrc/attn7p.hip), on the CPU: the two sources are compiled to gfx950
assembly with csrc/build.sh's flags (hipcc -S --cuda-device-only) and read back.

Printed:
  * per kernel instantiation the VGPR count and the scratch size (the .amdhsa metadata: .vgpr_count, .private_segment_fixed_size);
  * for the default long-key kernel att7p::attn7p_kernel<true, false, 16, SLIM, LEAN> under each body of the MF = 16 tile (LEAN = false: the
    first body; true: the lean one, option attn_tile16_lean) and, third column, under the slim key loop around the lean body (SLIM,
    option attn7p_slim) the HOT PATH of one iteration of the key loop, by instruction class.  One
    iteration = two 64-key tiles = 128 MFMAs and the DMA requests of the next two (full) tiles.  The hot path is the cheapest walk
    through the loop's blocks from its header back to its header that issues exactly 128 MFMAs and 8 global_load_lds: the re-base
    branches, the tail mask, the ragged-tile DMA and the piece-boundary code all cost instructions and carry no MFMA, so the cheapest
    walk leaves them out.

    python tools/attn_isa_census.py [--out FILE] [--keep DIR]
tests/test_attn_isa_census_cpu.py runs the same functions and asserts: no scratch and <= 256 VGPRs anywhere, no packed f32 VALU in
the lean hot path, fewer VALU instructions in it than in the first body's."""
import argparse
import heapq
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "infinicube_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SOURCES = ("attn7", "attn7p")
N_MFMA, N_DMA = 128, 8          # one iteration of the default long-key loop (8 waves: 2 K + 2 V DMA instructions per wave and tile)


def build_flags():
    """FLAGS=(...) of csrc/build.sh, with its $root / $here resolved: the census must see what the library is built from."""
    text = open(os.path.join(CSRC, "build.sh")).read()
    m = re.search(r"^FLAGS=\((.*)\)$", text, re.M)
    assert m, "csrc/build.sh: FLAGS=(...) not found"
    flags = [f.replace('"', "") for f in m.group(1).split()]
    return [f.replace("$root", ROOT).replace("$here", CSRC) for f in flags]


def compile_asm(src, outdir):
    out = os.path.join(outdir, src + ".s")
    cmd = [HIPCC] + build_flags() + ["-S", "--cuda-device-only", os.path.join(CSRC, src + ".hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)}\n{r.stderr}")
    return out


def compile_all(outdir):
    with ThreadPoolExecutor(len(SOURCES)) as ex:
        return dict(zip(SOURCES, ex.map(lambda s: compile_asm(s, outdir), SOURCES)))


def demangle(names):
    filt = os.path.join(os.path.dirname(os.path.realpath(HIPCC)), "..", "llvm", "bin", "llvm-cxxfilt")
    for tool in (filt, "/opt/rocm/llvm/bin/llvm-cxxfilt", "c++filt"):
        try:
            r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True)
            return dict(zip(names, r.stdout.split("\n")))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def kernel_resources(asm_text):
    """{mangled name: {"vgpr", "agpr", "scratch", "lds"}} from the amdhsa.kernels metadata at the end of the file."""
    out = {}
    meta = asm_text[asm_text.rindex("amdhsa.kernels:"):] if "amdhsa.kernels:" in asm_text else ""
    for entry in re.split(r"\n  - \.", meta)[1:]:
        f = dict(re.findall(r"^\s*\.?(\w+):\s+(\S+)\s*$", "." + entry, re.M))
        if "name" in f:
            out[f["name"]] = {"vgpr": int(f["vgpr_count"]), "agpr": int(f.get("agpr_count", 0)),
                              "scratch": int(f["private_segment_fixed_size"]), "lds": int(f.get("group_segment_fixed_size", 0))}
    return out


def function_blocks(asm_text, name):
    """The function's basic blocks in layout order: [(label, [instructions])]; a block ends at a label or behind a branch."""
    m = re.search(r"^" + re.escape(name) + r":.*?$(.*?)^\.Lfunc_end", asm_text, re.M | re.S)
    assert m, name + ": not in the assembly"
    blocks, n_anon = [("entry", [])], 0
    for line in m.group(1).split("\n"):
        lab = re.match(r"^(\.LBB\d+_\d+):", line)
        if lab:
            blocks.append((lab.group(1), []))
            continue
        ins = re.sub(r"\s*;.*", "", line).strip()
        if not ins or ins.startswith(".") or ins.endswith(":"):
            continue
        blocks[-1][1].append(ins)
        if re.match(r"s_c?branch|s_endpgm", ins):
            n_anon += 1
            blocks.append((f"anon{n_anon}", []))
    return blocks


def successors(blocks):
    index = {lab: i for i, (lab, _) in enumerate(blocks)}
    succ = []
    for i, (_, ins) in enumerate(blocks):
        last = ins[-1] if ins else ""
        nxt = [i + 1] if i + 1 < len(blocks) else []
        if last.startswith("s_branch"):
            succ.append([index[last.split()[-1]]])
        elif last.startswith("s_cbranch"):
            succ.append([index[last.split()[-1]]] + nxt)
        elif last.startswith("s_endpgm"):
            succ.append([])
        else:
            succ.append(nxt)
    return succ


def count(ins, pattern):
    return sum(1 for x in ins if re.match(pattern, x))


def hot_path(blocks, any_back_edge=False):
    """Instructions of the cheapest header-to-header walk with N_MFMA MFMAs and N_DMA LDS-DMA requests, over every candidate header:
    every target of a backward conditional branch; any_back_edge: of a backward s_branch as well (the steady loop of the slim form has
    its last re-base block laid out in front of its header, closes with an s_branch around it and reaches the header by falling through)."""
    succ = successors(blocks)
    cost = [(len(ins), count(ins, "v_mfma"), count(ins, "global_load_lds")) for _, ins in blocks]
    headers = sorted({t for i, s in enumerate(succ) for t in s if t <= i and blocks[i][1] and re.match(r"s_c?branch" if any_back_edge else r"s_cbranch", blocks[i][1][-1])})
    best = None
    for h in headers:
        start = (cost[h][0], h, cost[h][1], cost[h][2])
        heap, seen, prev = [start], set(), {start[1:]: None}
        while heap:
            c, b, nm, nd = heapq.heappop(heap)
            if (b, nm, nd) in seen:
                continue
            seen.add((b, nm, nd))
            for t in succ[b]:
                if t == h:
                    if nm == N_MFMA and nd == N_DMA and (best is None or c < best[0]):
                        path, k = [], (b, nm, nd)
                        while k is not None:
                            path.append(k[0])
                            k = prev[k]
                        best = (c, path[::-1])
                    continue
                k = (t, nm + cost[t][1], nd + cost[t][2])
                if k[1] > N_MFMA or k[2] > N_DMA or k in seen:
                    continue
                prev.setdefault(k, (b, nm, nd))
                heapq.heappush(heap, (c + cost[t][0], *k))
    assert best, "no loop iteration with %d MFMAs and %d LDS-DMA requests found" % (N_MFMA, N_DMA)
    return [x for b in best[1] for x in blocks[b][1]]


CLASSES = [          # first match wins
    ("v_mfma_f32_16x16x32_bf16", r"v_mfma_f32_16x16x32_bf16"),
    ("other v_mfma", r"v_mfma"),
    ("ds_read_b128", r"ds_read_b128"),
    ("ds_read_b64_tr_b16", r"ds_read_b64_tr_b16"),
    ("other ds_", r"ds_"),
    ("global_load_lds (DMA)", r"global_load_lds"),
    ("v_exp_f32", r"v_exp_f32"),
    ("v_cvt_pk_bf16_f32", r"v_cvt_pk_bf16_f32"),
    ("v_pk_*_f32 (packed f32)", r"v_pk_\w+_f32"),
    ("v_add_f32 / v_sub_f32", r"v_(add|sub|subrev)_f32"),
    ("other f32 VALU (mul, fma, max ...)", r"v_(mul|fma|fmac|max|max3|min|mad)_f32"),
    ("v_mov_b32 / v_mov_b64", r"v_mov_b(32|64)"),
    ("v_cmp / v_cndmask", r"v_(cmp|cmpx|cndmask)"),
    ("v_readfirstlane / v_readlane", r"v_read"),
    ("integer VALU (v_add_u32, shifts, logic ...)", r"v_"),
    ("s_nop", r"s_nop"),
    ("s_waitcnt", r"s_waitcnt"),
    ("s_barrier / s_setprio", r"s_(barrier|setprio)"),
    ("branches", r"s_c?branch"),
    ("other SALU", r"s_"),
    ("other", r""),
]


def classify(ins):
    out = {name: 0 for name, _ in CLASSES}
    for x in ins:
        for name, pat in CLASSES:
            if re.match(pat, x):
                out[name] += 1
                break
    out["VALU total (v_* without MFMA)"] = count(ins, r"v_(?!mfma)")
    out["instructions"] = len(ins)
    return out


def default_kernel(resources, lean, slim=False):
    """Mangled name of att7p::attn7p_kernel<true, false, 16, slim, lean> (before the slim loop existed: <true, false, 16, lean>; before
    the lean body: <true, false, 16>)."""
    assert lean or not slim
    hits = [n for n in resources if "attn7p_kernel" in n and "ILb1ELb0ELi16ELb%dELb%dEEE" % (slim, lean) in n]
    if not hits and not slim:
        hits = [n for n in resources if "attn7p_kernel" in n and "ILb1ELb0ELi16ELb%dEEE" % lean in n]
    if not hits and not lean:
        hits = [n for n in resources if "attn7p_kernel" in n and "ILb1ELb0ELi16EEE" in n]
    assert len(hits) == 1, f"attn7p_kernel<true, false, 16, {slim}, {lean}>: {hits}"
    return hits[0]


def census(outdir):
    """{"resources": {source: {demangled: {...}}}, "hot": {"first": {...}, "lean": {...}, "slim": {...}}}"""
    asm = {s: open(p).read() for s, p in compile_all(outdir).items()}
    res, result = {}, {"resources": {}, "hot": {}}
    for s, text in asm.items():
        res[s] = kernel_resources(text)
        names = demangle(list(res[s]))
        result["resources"][s] = {names[n]: r for n, r in res[s].items()}
    for arm, lean, slim in (("first", False, False), ("lean", True, False), ("slim", True, True)):
        name = default_kernel(res["attn7p"], lean, slim)
        result["hot"][arm] = classify(hot_path(function_blocks(asm["attn7p"], name), any_back_edge=slim))
    return result


def report(c):
    lines = ["VGPRs, AGPRs and scratch bytes per instantiation (hipcc -S with csrc/build.sh's flags)", ""]
    for s in SOURCES:
        lines.append(f"csrc/{s}.hip")
        for n, r in sorted(c["resources"][s].items()):
            lines.append(f"  vgpr {r['vgpr']:3d}  agpr {r['agpr']:3d}  scratch {r['scratch']:4d} B  {n}")
        lines.append("")
    lines += ["hot path of one iteration of the key loop (two 64-key tiles, 128 keys) of att7p::attn7p_kernel<true, false, 16, SLIM, LEAN>",
              "  first = LEAN false (attn_tile16_lean = 0), lean = LEAN true (attn_tile16_lean = 1),",
              "  slim = LEAN and SLIM true (attn7p_slim = 1): the steady interval of the slim key loop", "",
              f"  {'instructions per 128 keys':46s} {'first':>6s} {'lean':>6s} {'slim':>6s}"]
    for k in c["hot"]["first"]:
        lines.append(f"  {k:46s} {c['hot']['first'][k]:6d} {c['hot']['lean'][k]:6d} {c['hot']['slim'][k]:6d}")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--keep", default=None, help="keep the assembly in this directory")
    a = ap.parse_args()
    if a.keep:
        os.makedirs(a.keep, exist_ok=True)
        text = report(census(a.keep))
    else:
        with tempfile.TemporaryDirectory() as d:
            text = report(census(d))
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
