#!/usr/bin/env python3
"""Generates tests/golden/diffsynth_shim_reference.npz: the frames, the printed progress lines and the model configs
that the REFERENCE wrapper (/root/reference/infinicube/videogen/inference.py, loaded by path, nothing is copied) produces
on top of this repo's `diffsynth` shim, with `from_pretrained` pointed at the tiny in-memory pipeline of
tests/mgpu_factory.py.  tests/test_diffsynth_shim.py compares this repo's own WanVideoGenerator against it.
Run in the build container only (needs /root/reference):  python tests/golden/make_diffsynth_shim_golden.py
"""
import contextlib
import importlib.util
import io
import json
import os
import sys
import tempfile

import numpy as np
from safetensors.torch import save_file

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [os.path.dirname(TESTS), TESTS]
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
REF_FILE = "/root/reference/infinicube/videogen/inference.py"
OUT = os.path.join(HERE, "diffsynth_shim_reference.npz")


def main():
    import diffsynth.pipelines.wan_video_new as shim
    import mgpu_factory as F
    from infinicube_amd.videogen import synthetic as syn
    seen = {}

    def from_pretrained(torch_dtype=None, device=None, model_configs=None, **kw):
        seen["configs"] = [(m.model_id, m.origin_file_pattern, m.skip_download) for m in model_configs]
        return F.factory(torch_dtype, device, model_configs)

    shim.WanVideoPipeline.from_pretrained = staticmethod(from_pretrained)
    spec = importlib.util.spec_from_file_location("ref_videogen_inference", REF_FILE)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)            # imports `diffsynth` -> the shim
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "step-1.safetensors")
    save_file({"buffer_embedder." + k: v for k, v in syn.make_buffer_embedder_state_dict(F.CFG).items()}, path)
    sem, co = syn.make_dummy_buffers(F.GRID)
    out = os.path.join(tmp, "video_480p_front.mp4")
    with contextlib.redirect_stdout(io.StringIO()) as log:
        g = ref.WanVideoGenerator(path, device="cpu", use_wan_1pt3b=True)
        frames = g.generate(sem, co, seed=0, output_path=out)
    assert os.path.getsize(out) > 0
    np.savez_compressed(OUT, frames=np.stack([np.asarray(f) for f in frames]), log=np.array(log.getvalue().replace(tmp, "<tmp>")),
                        configs=np.array(json.dumps(seen["configs"])))
    print("wrote", OUT)


if __name__ == "__main__":
    main()
