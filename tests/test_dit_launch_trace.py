"""The launch sequence of dit.WanDiT.denoise, pinned: for every driver mode that runs on the CPU operator set (sequential /
CFG-batched forwards x shared stem, sequence-parallel rehearsal, e4m3 operands and wire format, i2v, TeaCache, the cfg+sp
loop) the ordered list of ops with the rows of the buffers they touch (tests/dit_launch_trace.py) must hash to what
tests/golden/dit_launch_trace.json recorded on the commit named in its header, and so must the latent the loop leaves."""
import json
import os

import pytest

import dit_launch_trace as T

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dit_launch_trace.json")) as f:
    GOLDEN = json.load(f)


def test_golden_covers_exactly_the_cases():
    assert set(GOLDEN["cases"]) == set(T.cases())
    assert len(GOLDEN["header"]["generated_on_commit"]) == 40


@pytest.mark.parametrize("name", sorted(T.cases()))
def test_launch_trace_equals_golden(name):
    got, want = T.summarize(*T.run_case(*T.cases()[name])), GOLDEN["cases"][name]
    moved = {op: (want["histogram"].get(op, 0), got["histogram"].get(op, 0))
             for op in sorted(set(want["histogram"]) | set(got["histogram"])) if want["histogram"].get(op, 0) != got["histogram"].get(op, 0)}
    assert not moved, f"launch counts changed, op: (golden, now) = {moved}"
    assert got["ops"] == want["ops"]
    assert got["log_sha256"] == want["log_sha256"], "same ops, but their order or the buffers / rows they run on changed"
    assert got["latent_sha256"] == want["latent_sha256"]
