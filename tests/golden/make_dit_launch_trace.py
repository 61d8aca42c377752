#!/usr/bin/env python3
"""Generates tests/golden/dit_launch_trace.json: per case of tests/dit_launch_trace.py the op count, the per-op-name
histogram and the SHA-256 of the launch log and of the final latent of dit.WanDiT.denoise on the CPU operator set.

The golden pins the launch sequence across changes of the host driver, so it is generated on the commit BEFORE such a change
and the changed driver is tested against it:
    python tests/golden/make_dit_launch_trace.py <hash of the commit the working tree's dit.py comes from>
``--dump DIR`` additionally writes every case's full log as DIR/<case>.json, to diff two drivers entry by entry."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import dit_launch_trace as T  # noqa: E402


def main(argv):
    dump = None
    if "--dump" in argv:
        i = argv.index("--dump")
        dump = argv[i + 1]
        del argv[i:i + 2]
        os.makedirs(dump, exist_ok=True)
    if len(argv) != 2:
        sys.exit(__doc__)
    out = {"header": {"generated_on_commit": argv[1],
                      "note": "produced by tests/golden/make_dit_launch_trace.py on the commit named here, the parent of the "
                              "change that gave the transformer block ONE schedule for single and CFG-paired forwards; "
                              "NOT regenerated from the refactored driver"},
           "cases": {}}
    for name, case in T.cases().items():
        log, lat = T.run_case(*case)
        out["cases"][name] = T.summarize(log, lat)
        if dump:
            with open(os.path.join(dump, name.replace("/", "__") + ".json"), "w") as f:
                json.dump(log, f, indent=0)
        print(name, out["cases"][name]["ops"], out["cases"][name]["log_sha256"][:12])
    with open(os.path.join(HERE, "dit_launch_trace.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(list(sys.argv))
