"""The score constructions, the float64 bounds and the lazy-max emulator of tests/attn_scores.py, on the CPU.

(a) every construction is what it claims (exact in bf16 and e4m3, margins, the staircase's re-base tiles);
(b) the bounds hold on the emulated loop for every construction, thr in {0, 8}, one launch and carried-state chunks;
(c) every mutant of the loop (attn_scores.MUTATIONS) is rejected by at least one of the assertions the GPU tests make -
    the evidence that those bars can catch a real kernel bug."""
import pytest
import torch

import attn_scores as A

SKV = 700            # 11 tiles, ragged tail of 60 keys
CHUNKS = ([SKV], [130, 493, 77])


def cases(Sq=70, Skv=SKV, H=2):
    return [
        A.one_hot(Sq, Skv, H, [0, Skv - 1, 63, 64, 127, 128, 383, 384, 640], seed=1),
        A.staircase(Sq, Skv, H, [1, 2, 3, 5, 10], seed=2),
        A.staircase(Sq, Skv, H, [10], seed=3),
        A.falling(Sq, Skv, H, seed=4),
        A.mixed_rows(Sq, Skv, H, seed=5),
        A.temperature(Sq, Skv, H, 8.0, seed=6),
        A.temperature(Sq, Skv, H, 16.0, seed=7),
        A.ties(Sq, Skv, H, seed=8),
    ]


def all_checks(c, fp8, thr, chunks, mutation=None):
    """Every assertion the GPU tests make, on the emulator's output and carried states: the list of failures."""
    H = c["q"].shape[1] // A.D
    s, ds = A.scores(c["q"], c["k"], H, fp8=fp8)
    vh = A.heads_v(c["v"], H, fp8=fp8)
    o, states, reb = A.emulate(s, vh, chunks, thr, fp8=fp8, mutation=mutation)
    what = f"{c['name']} fp8={fp8} thr={thr} chunks={chunks} mutation={mutation}"
    f = A.check_output(o, s, ds, vh, fp8, len(chunks), what=what)
    f += A.check_suite_bar(o, s, vh, what=what) if not fp8 else []
    for acc, ml, kk in states:
        f += A.check_state(s[..., :kk], ds, vh[:, :kk], acc, ml, thr, fp8=fp8, chunks=len(chunks), what=what + f" state@{kk}")
    if "dom" in c and not torch.equal(o, A.expected_one_hot(c, H, fp8)):
        f.append(what + ": one-hot not bit-exact")
    return f, reb


@pytest.mark.parametrize("fp8", [False, True])
def test_constructions_are_exact(fp8):
    for c in cases():
        H = c["q"].shape[1] // A.D
        for t in (c["q"], c["k"], c["v"]):
            if c["name"].startswith("temp"):
                continue
            assert A.is_fp8_exact(t, H), f"{c['name']}: not exact in e4m3 after the head's scale"
        if c["name"].startswith("temp"):
            continue
        s, ds = A.scores(c["q"], c["k"], H, fp8=fp8)
        assert torch.equal(s, torch.round(s)) and float(s.abs().max()) <= A.S_MAX and float(ds.max()) < 1e-3
        # the score the profile names is the score the inputs give (every head)
        assert torch.equal(s[0], c["profiles"][c["group"]].double()) and torch.equal(s[-1], s[0])
        if c["name"] == "one_hot":
            srt = s.sort(-1, descending=True).values
            assert float((srt[..., 0] - srt[..., 1]).min()) >= 80
            assert torch.equal(s.argmax(-1)[0], c["dom"])
    assert bool((A.v_values(1000, 2, 0).float() != 0).all())


def test_temperature_scores_have_the_named_spread():
    c = A.temperature(64, 2000, 1, 8.0, seed=11)
    s, _ = A.scores(c["q"], c["k"], 1)
    centred = s - s.mean(-1, keepdim=True)
    std_nat = float(centred.std()) / A.math.log2(A.math.e)
    assert 6.0 < std_nat < 10.0
    off = s.mean(-1)[0]
    assert float(off.abs().max()) > 150           # rows sit far from 0 ...
    assert float((centred.amax(-1) - centred.amin(-1)).min()) > 30   # ... and are sharply peaked


@pytest.mark.parametrize("fp8", [False, True])
def test_staircase_rebases_exactly_at_the_named_tiles(fp8):
    for rises in ([1, 2, 3, 4, 5, 6, 7, 8, 9, 10], [2, 4, 6, 8, 10], [10], [3, 7]):
        c = A.staircase(40, SKV, 1, rises)
        for thr in (0, 8):
            for chunks in CHUNKS:
                _, reb = all_checks(c, fp8, thr, chunks)
                for r in range(40):
                    assert sorted(reb[0][r]) == c["rises"], (rises, thr, chunks, sorted(reb[0][r]))


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("thr", [0, 8])
def test_bounds_hold_on_the_emulated_loop(fp8, thr):
    for c in cases():
        for chunks in CHUNKS:
            f, _ = all_checks(c, fp8, thr, chunks)
            assert not f, f


def test_thr0_state_m_is_the_true_max():
    c = A.staircase(40, SKV, 1, [2, 5, 9])
    s, _ = A.scores(c["q"], c["k"], 1)
    vh = A.heads_v(c["v"], 1)
    _, states, _ = A.emulate(s, vh, [130, 493, 77], 0)
    for acc, ml, kk in states:
        assert torch.equal(ml[:, 0, 0].double(), s[0, :, :kk].amax(-1))


@pytest.mark.parametrize("mutation", A.MUTATIONS)
@pytest.mark.parametrize("fp8", [False, True])
def test_mutants_are_rejected(mutation, fp8):
    caught = []
    for c in cases():
        for thr in (0, 8):
            for chunks in CHUNKS:
                f, _ = all_checks(c, fp8, thr, chunks, mutation=mutation)
                caught += f
    assert caught, f"mutant {mutation} (fp8={fp8}) passed every assertion"
