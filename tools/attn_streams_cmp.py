"""Are the instruction streams of the attention kernels what they were?  Two directories of gfx950 assembly of csrc/attn7.hip and
csrc/attn7p.hip (tools/attn_isa_census.py --keep DIR, once on the older commit and once on this one) are compared function by
function: every kernel of the older build must be in the newer one with the same instructions in the same order.  Block labels
are compared by their number inside the function (the function's index in the file is part of a label's text and moves when a
kernel is added).  Kernels are matched by demangled name; a template parameter the newer build added is passed as
--drop INDEX=VALUE (attn7p_kernel<UNIT, FW, MF, SLIM, LEAN>: --drop 3=false names what <UNIT, FW, MF, LEAN> was).

    python tools/attn_streams_cmp.py OLD_DIR NEW_DIR [--drop 3=false] [--out FILE]
Exit status 1 if a kernel is missing or differs."""
import argparse
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_isa_census as C  # noqa: E402


def stream(asm_text, name):
    ins = [x for _, b in C.function_blocks(asm_text, name) for x in b]
    return [re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", x) for x in ins]


def old_name(demangled, drop):
    """The name this kernel had before the parameters in `drop` {index: value} existed; None if it is a new instantiation."""
    m = re.match(r"(.*attn7p_kernel<)([^>]*)(>.*)", demangled)
    if not m or not drop:
        return demangled
    args = [a.strip() for a in m.group(2).split(",")]
    for i in sorted(drop, reverse=True):
        if i >= len(args) or args[i] != drop[i]:
            return None
        del args[i]
    return m.group(1) + ", ".join(args) + m.group(3)


def compare(old_dir, new_dir, drop):
    lines, bad, n_same, n_new = [], 0, 0, 0
    for src in C.SOURCES:
        old = open(os.path.join(old_dir, src + ".s")).read()
        new = open(os.path.join(new_dir, src + ".s")).read()
        old_k, new_k = list(C.kernel_resources(old)), list(C.kernel_resources(new))
        old_d, new_d = C.demangle(old_k), C.demangle(new_k)
        by_old = {}
        for n in new_k:
            was = old_name(new_d[n], drop)
            if was is None:
                n_new += 1
                lines.append(f"new   {len(stream(new, n)):6d} instructions  {new_d[n]}")
            else:
                by_old[was] = n
        for o in sorted(old_k, key=lambda k: old_d[k]):
            n = by_old.get(old_d[o])
            if n is None:
                bad += 1
                lines.append(f"GONE                        {old_d[o]}")
                continue
            a, b = stream(old, o), stream(new, n)
            if a == b:
                n_same += 1
                lines.append(f"same  {len(a):6d} instructions  {old_d[o]}")
            else:
                bad += 1
                first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
                lines.append(f"DIFF  {len(a):6d} -> {len(b):6d}, first at {first}  {old_d[o]}")
    head = [f"{n_same} kernels with the older build's instruction stream, {bad} that differ or are gone, {n_new} new instantiations", ""]
    return "\n".join(head + lines) + "\n", bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old_dir")
    ap.add_argument("new_dir")
    ap.add_argument("--drop", action="append", default=[], help="INDEX=VALUE: an attn7p_kernel template parameter the newer build added")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    drop = {int(d.split("=")[0]): d.split("=")[1] for d in a.drop}
    text, bad = compare(a.old_dir, a.new_dir, drop)
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
