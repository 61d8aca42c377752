"""SURVEY.md §8f row 1 — coordinate guidance buffer.  This oracle IS pinned: the golden arrays in
tests/golden/coord_buffer_cases.npz are outputs of the reference's own function (generator:
tests/golden/make_coord_buffer_golden.py).  CPU: oracle vs reference golden.  GPU: HIP path (C ABI) vs
golden and vs the oracle at the full 93x480x832 size through size-independent properties.
Ragged widths, rows wider than a block, unaligned pointers and the other edges of these kernels: tests/test_buffer_edges_gpu.py."""
import os

import numpy as np
import pytest
import torch

from oracle import buffer_ref as B

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "coord_buffer_cases.npz"))
CASES = ("small", "allsky", "big")


class Cam:
    def __init__(self, fx, fy, cx, cy):
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)

    def get_intrinsics_matrix(self):
        return torch.tensor([[self.fx, 0, self.cx], [0, self.fy, self.cy], [0, 0, 1]], dtype=torch.float32)


def _case(name):
    return (torch.from_numpy(G[f"{name}_depth"]), torch.from_numpy(G[f"{name}_poses"]), Cam(*G[f"{name}_intr"]),
            int(G[f"{name}_seed"][0]), torch.from_numpy(G[f"{name}_coord"]), G[f"{name}_coord_u8"])


@pytest.mark.parametrize("name", CASES)
def test_oracle_matches_reference_golden(name):
    depth, poses, cam, seed, want, _ = _case(name)
    torch.manual_seed(seed)
    got = B.coordinate_buffer_global_norm(depth, cam.get_intrinsics_matrix(), poses, 0.05)
    assert float((got - want).abs().max()) < 1e-6


def test_oracle_unproject_identity_pose():
    depth = torch.full((1, 4, 6), 2.0)
    k = torch.tensor([[10.0, 0, 3.0], [0, 10.0, 2.0], [0, 0, 1]])
    pts = B.unproject_depth(depth, torch.eye(4)[None], k[None])
    assert torch.allclose(pts[0, 2, 3], torch.tensor([0.0, 0.0, 2.0]))          # principal point -> on the optical axis
    assert torch.allclose(pts[0, 2, 5], torch.tensor([0.4, 0.0, 2.0]))          # 2 px right at depth 2, f = 10


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_hip_kernels_bit_exact_from_reference_host_values(name):
    """The per-pixel byte work, pinned bit for bit: the three HIP kernels (through the C ABI) fed the few numbers the
    reference derives on the host (K^-1, pose_0^-1 pose_n, the sample quantiles - stored in the golden file by the
    generator script from the reference's own torch calls) must reproduce the reference's float32 buffer AND the
    caller's uint8 buffer exactly.  (Those host numbers come from LAPACK / BLAS and differ in the last bit between CPU
    models - this test is independent of the host it runs beside; the function-level test below is not.)"""
    import ctypes
    from infinicube_amd import native
    lib = native.lib()
    depth = torch.from_numpy(G[f"{name}_depth"]).to("cuda:0")
    n, h, w = depth.shape
    cf = lambda a: (ctypes.c_float * a.size)(*[float(x) for x in a.reshape(-1)])   # noqa: E731
    kinv, tf = cf(G[f"{name}_kinv"]), torch.from_numpy(G[f"{name}_to_cam0"]).contiguous().to("cuda:0")
    mins, ranges, hv = cf(G[f"{name}_mins"]), cf(G[f"{name}_ranges"]), int(G[f"{name}_has_valid"][0])
    of = torch.empty((n, h, w, 3), dtype=torch.float32, device="cuda:0")
    ou = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    native.check(lib.icv_coord_normalize(depth.data_ptr(), kinv, tf.data_ptr(), n, h, w, mins, ranges, hv, of.data_ptr(), ou.data_ptr(), st))
    torch.cuda.synchronize()
    assert np.array_equal(of.cpu().numpy(), G[f"{name}_coord"]), "float32 coordinate buffer differs from the reference's"
    assert np.array_equal(ou.cpu().numpy(), G[f"{name}_coord_u8"]), "uint8 coordinate buffer differs from the reference's"
    # the valid mask and the gathered sample points are the reference's too (flattened order)
    mask = torch.empty((n * h * w,), dtype=torch.uint8, device="cuda:0")
    native.check(lib.icv_coord_valid_mask(depth.data_ptr(), kinv, tf.data_ptr(), n, h, w, mask.data_ptr(), st))
    want_mask = B.coord_valid_mask_f32(G[f"{name}_depth"], G[f"{name}_kinv"], G[f"{name}_to_cam0"])
    assert np.array_equal(mask.cpu().numpy().reshape(n, h, w), want_mask), "valid mask differs from the restatement's, pixel by pixel"


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_hip_matches_reference_golden(name):
    from infinicube.utils.buffer_utils import generate_coordinate_buffer_from_memory_global_norm as gen
    depth, poses, cam, seed, want, want_u8 = _case(name)
    # does THIS host's LAPACK reproduce the host-side numbers of the machine the golden was made on?
    k = cam.get_intrinsics_matrix()
    same_host_math = (np.array_equal(torch.inverse(k).numpy(), G[f"{name}_kinv"]) and np.array_equal(
        torch.einsum("ij,bjk->bik", torch.inverse(poses[0]), poses).numpy(), G[f"{name}_to_cam0"]))
    torch.manual_seed(seed)
    got = gen(depth, cam, poses, percentile=0.05, sampling="reference").cpu()
    assert got.shape == want.shape and got.dtype == torch.float32
    torch.manual_seed(seed)
    u8 = gen(depth, cam, poses, percentile=0.05, return_uint8=True, sampling="reference").cpu().numpy()
    if same_host_math:
        assert torch.equal(got, want), f"coordinate buffer differs from the reference's output: max {float((got - want).abs().max())}"
        assert np.array_equal(u8, want_u8), "the uint8 coordinate buffer must match the reference byte for byte"
    else:   # another CPU model: K^-1 / pose products differ in the last bit, so does everything downstream
        print(f"[{name}] host inverse/einsum differ from the golden's host in the last bit: comparing within 4 ulp")
        assert float((got - want).abs().max()) <= 4 * 2.0 ** -24
        diff = np.abs(u8.astype(np.int16) - want_u8.astype(np.int16))
        assert diff.max() <= 1 and (diff > 0).mean() < 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_hip_device_sampling_vs_reference_golden(name):
    """The default ``sampling="device"`` path (round 6; opt-in before) draws the <= 100000-point quantile sample on the device (stratified, unseeded like the
    reference's own draw): with <= 100000 finite points ("small", "allsky") the sample is every finite point and the bytes
    equal the reference's; with more ("big": 118 640) the two 100000-point samples differ by design and the quantile
    estimates with them — bar: every uint8 within +-1 of the reference's output, at most 2 % of the bytes off by one."""
    from infinicube.utils.buffer_utils import generate_coordinate_buffer_from_memory_global_norm as gen
    depth, poses, cam, seed, want, want_u8 = _case(name)
    k = cam.get_intrinsics_matrix()
    same_host_math = (np.array_equal(torch.inverse(k).numpy(), G[f"{name}_kinv"]) and np.array_equal(
        torch.einsum("ij,bjk->bik", torch.inverse(poses[0]), poses).numpy(), G[f"{name}_to_cam0"]))
    u8 = gen(depth, cam, poses, percentile=0.05, return_uint8=True, sampling="device").cpu().numpy()   # the device-side draw (the default)
    diff = np.abs(u8.astype(np.int16) - want_u8.astype(np.int16))
    frac = float((diff > 0).mean())
    print(f"[{name}] device-sampled coordinate buffer vs the reference's bytes: max |diff| {diff.max()}, {100 * frac:.3f} % of bytes differ")
    if int((G[f"{name}_depth"] != 0).sum()) <= 100000 and same_host_math:
        assert diff.max() == 0
    else:
        # the yardstick is the reference against ITSELF: its draw is unseeded, so two of its own runs differ by the sampling
        # noise of two 100000-point quantile estimates - a shift of ~1e-3 of the range moves ~255e-3 of all bytes across a
        # rounding boundary.  The device sample must sit inside that spread: every byte within +-1, and no more bytes off by
        # one than twice what the reference's own second draw shows (+ 2 % slack).
        torch.manual_seed(seed + 1)
        other = gen(depth, cam, poses, percentile=0.05, return_uint8=True, sampling="reference").cpu().numpy()
        d_ref = np.abs(other.astype(np.int16) - want_u8.astype(np.int16))
        frac_ref = float((d_ref > 0).mean())
        print(f"[{name}] the reference's algorithm under another seed vs its golden run: max |diff| {d_ref.max()}, {100 * frac_ref:.3f} % of bytes differ")
        assert diff.max() <= 1 and frac <= 2.0 * frac_ref + 0.02, f"device sample outside the reference's own run-to-run spread: {frac} vs {frac_ref}"
    f32 = gen(depth, cam, poses, percentile=0.05, sampling="device").cpu()
    assert float((f32 - want).abs().max()) <= 2.0 / 255.0


@pytest.mark.gpu
def test_hip_full_size_properties():
    """93 x 480 x 832 (the BASELINE configs' buffer size): range, sky, monotonicity in depth along the optical
    axis, and invariance to a rigid motion applied to ALL poses (only relative poses matter)."""
    from infinicube_amd.utils.buffer_utils import generate_coordinate_buffer_from_memory_global_norm as gen
    n, h, w = 93, 480, 832
    g = torch.Generator().manual_seed(0)
    depth = torch.rand((n, h, w), generator=g) * 60 + 2
    depth[:, :100] = 0                                                       # sky rows
    poses = torch.eye(4).repeat(n, 1, 1)
    poses[:, 2, 3] = torch.arange(n) * 0.5
    cam = Cam(700.0, 700.0, w / 2, h / 2)
    gdev = torch.Generator(device="cuda:0")
    gdev.manual_seed(5)
    a = gen(depth, cam, poses, generator=gdev, sampling="device")
    assert a.shape == (n, h, w, 3) and float(a.min()) >= 0.0 and float(a.max()) <= 1.0
    assert bool((a[:, :100] == 1.0).all())
    rigid = torch.tensor([[0.0, -1.0, 0.0, 5.0], [1.0, 0.0, 0.0, -3.0], [0.0, 0.0, 1.0, 2.0], [0.0, 0.0, 0.0, 1.0]])
    gdev.manual_seed(5)
    b = gen(depth, cam, torch.einsum("ij,njk->nik", rigid, poses), generator=gdev, sampling="device")
    assert float((a - b).abs().max()) < 1e-4
    gdev.manual_seed(5)
    u8 = gen(depth, cam, poses, return_uint8=True, generator=gdev, sampling="device")
    assert u8.dtype == torch.uint8 and torch.equal(u8, (a * 255).to(torch.uint8))
    # against the reference's host-RNG sampling on the same input, with the reference's own run-to-run spread (two seeds) as
    # the yardstick: every byte within +-1, and no more bytes off by one than twice what two of its own draws show
    refs = []
    for sd in (5, 6):
        torch.manual_seed(sd)
        refs.append(gen(depth, cam, poses, return_uint8=True, sampling="reference").to(torch.int16))
    d_rr = (refs[0] - refs[1]).abs()
    d8 = (u8.to(torch.int16) - refs[0]).abs()
    f_rr, f_dev = float((d_rr > 0).float().mean()), float((d8 > 0).float().mean())
    print(f"93x480x832: device vs reference sampling {100 * f_dev:.2f} % of bytes differ (max {int(d8.max())}); reference seed 5 vs seed 6: {100 * f_rr:.2f} % (max {int(d_rr.max())})")
    assert int(d8.max()) <= 1 and f_dev <= 2.0 * f_rr + 0.02, f"device vs reference sampling: max {int(d8.max())}, {100 * f_dev:.2f} % differ (reference vs itself {100 * f_rr:.2f} %)"


# ---------------------------------------------------------------------------------------------------
# §8f row 2: semantic / instance colour buffer (golden = the reference's own outputs, generator:
# tests/golden/make_semantic_golden.py; palette under the documented pycg == matplotlib assumption)
# ---------------------------------------------------------------------------------------------------
S = np.load(os.path.join(os.path.dirname(__file__), "golden", "semantic_buffer_cases.npz"))


def test_semantic_tables_match_reference():
    from infinicube_amd.utils import semantic_utils as su
    assert np.array_equal(su.WAYMO_MAPPING, S["mapping"]) and np.allclose(su.WAYMO_PALETTE, S["palette"])
    assert len(su.WAYMO_CATEGORY_NAMES) == 23


def test_semantic_oracle_matches_reference_golden():
    assert np.array_equal(B.semantic_to_color(S["sem"], S["mapping"], S["palette"]), S["colors"])
    np.random.seed(int(S["np_seed"][0]))
    assert np.array_equal(B.rgb_semantic_buffer(S["sem_rgb"], S["inst"]), S["rgb"])


@pytest.mark.gpu
def test_semantic_hip_matches_reference_golden():
    from infinicube.utils.semantic_utils import generate_rgb_semantic_buffer, semantic_to_color
    colors = semantic_to_color(S["sem"])
    assert colors.dtype == np.float32 and np.array_equal(colors, S["colors"])
    assert np.array_equal(semantic_to_color(torch.from_numpy(S["sem"])), S["colors"])     # tensor input, like the caller
    np.random.seed(int(S["np_seed"][0]))
    rgb = generate_rgb_semantic_buffer((colors * 255).astype(np.uint8), S["inst"])
    assert rgb.dtype == np.uint8 and np.array_equal(rgb, S["rgb"])
    # full-size property: pixels without an instance keep the semantic colour, bit for bit
    g = np.random.default_rng(3)
    sem_rgb = g.integers(0, 255, (93, 480, 832, 3), dtype=np.uint8)
    inst = np.zeros((93, 480, 832), np.uint16)
    inst[:, 100:200, 300:500] = 9
    inst[5:, 300:350, 100:150] = 2 ** 15 + 1
    out = generate_rgb_semantic_buffer(sem_rgb, inst)
    assert np.array_equal(out[inst == 0], sem_rgb[inst == 0])
    assert len(np.unique(out[inst == 9].reshape(-1, 3), axis=0)) == 1


@pytest.mark.gpu
def test_buffer_kernel_throughput_report(capsys):
    """Measurement, not a pass/fail bar (only sanity-bounded): HBM GB/s of the five guidance-buffer kernels at the
    BASELINE buffer size 93 x 480 x 832, with the CPU restatement of the reference functions (oracle/buffer_ref.py)
    timed beside them on this box's host.  The printed table is what profiles/r02/buffers.md holds."""
    import ctypes
    import time
    from infinicube_amd import native
    from infinicube_amd.utils import semantic_utils as su
    lib = native.lib()
    n, h, w = 93, 480, 832
    px = n * h * w
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    depth = torch.rand((n, h, w), generator=g) * 60 + 2
    depth[:, :100] = 0
    poses = torch.eye(4).repeat(n, 1, 1)
    poses[:, 2, 3] = torch.arange(n) * 0.5
    cam = Cam(700.0, 700.0, w / 2, h / 2)
    d_dev = depth.to(dev)
    cf = lambda a: (ctypes.c_float * len(a))(*[float(x) for x in a])   # noqa: E731
    kinv = cf(torch.inverse(cam.get_intrinsics_matrix()).reshape(-1).tolist())
    tf = poses.contiguous().to(dev)
    st = torch.cuda.current_stream().cuda_stream
    mask = torch.empty((px,), dtype=torch.uint8, device=dev)
    idx = torch.arange(0, px, px // 100000, device=dev)[:100000].contiguous()
    samp = torch.empty((idx.numel(), 3), device=dev)
    of, ou = torch.empty((n, h, w, 3), device=dev), torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    sem = torch.randint(0, 23, (px,), dtype=torch.int32, device=dev)
    lut = torch.from_numpy(su.WAYMO_PALETTE[su.WAYMO_MAPPING]).to(dev).contiguous()
    cf32 = torch.empty((px, 3), device=dev)
    inst = torch.zeros((px,), dtype=torch.int32, device=dev)
    inst[: px // 10] = 7
    ilut = torch.zeros((65536, 3), dtype=torch.uint8, device=dev)
    srgb = torch.randint(0, 255, (px, 3), dtype=torch.uint8, device=dev)
    orgb = torch.empty_like(srgb)
    du16 = torch.empty((px,), dtype=torch.uint16, device=dev)
    mins, rngs = cf([-10.0, -5.0, 0.0]), cf([20.0, 10.0, 80.0])
    cases = [
        ("icv_coord_valid_mask", lambda: lib.icv_coord_valid_mask(d_dev.data_ptr(), kinv, tf.data_ptr(), n, h, w, mask.data_ptr(), st), px * (4 + 1)),
        ("icv_coord_gather_points (100k samples)", lambda: lib.icv_coord_gather_points(d_dev.data_ptr(), kinv, tf.data_ptr(), n, h, w, idx.data_ptr(), idx.numel(), samp.data_ptr(), st), idx.numel() * (8 + 4 + 12)),
        ("icv_coord_normalize -> f32", lambda: lib.icv_coord_normalize(d_dev.data_ptr(), kinv, tf.data_ptr(), n, h, w, mins, rngs, 1, of.data_ptr(), None, st), px * (4 + 12)),
        ("icv_coord_normalize -> u8", lambda: lib.icv_coord_normalize(d_dev.data_ptr(), kinv, tf.data_ptr(), n, h, w, mins, rngs, 1, None, ou.data_ptr(), st), px * (4 + 3)),
        ("icv_semantic_to_color -> f32", lambda: lib.icv_semantic_to_color(sem.data_ptr(), px, lut.data_ptr(), 23, cf32.data_ptr(), None, st), px * (4 + 12)),
        ("icv_instance_overlay_u8", lambda: lib.icv_instance_overlay_u8(srgb.data_ptr(), inst.data_ptr(), px, ilut.data_ptr(), orgb.data_ptr(), st), px * (3 + 4 + 3)),
        ("icv_depth_to_u16", lambda: lib.icv_depth_to_u16(d_dev.data_ptr(), px, 100.0, du16.data_ptr(), st), px * (4 + 2)),
    ]
    lines = ["| kernel | bytes / call (algorithmic) | us / call | GB/s | % of 8 TB/s |", "|---|---|---|---|---|"]
    for name, fn, nbytes in cases:
        for _ in range(3):
            assert fn() == 0
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / 20
        gbs = nbytes / (us * 1e-6) / 1e9
        lines.append(f"| {name} | {nbytes / 1e6:.1f} MB | {us:.1f} | {gbs:.0f} | {100 * gbs / 8000:.1f} |")
        assert gbs > 50 or "gather" in name, f"{name}: {gbs:.0f} GB/s"
    # the reference's CPU path (restated: oracle/buffer_ref.py), a 6-frame sample scaled to 93 frames
    torch.manual_seed(0)
    t0 = time.perf_counter()
    B.coordinate_buffer_global_norm(depth[:6], cam.get_intrinsics_matrix(), poses[:6], 0.05)
    t_coord = (time.perf_counter() - t0) * n / 6
    semn = sem.cpu().numpy().reshape(n, h, w)
    t0 = time.perf_counter()
    B.semantic_to_color(semn[:6], su.WAYMO_MAPPING, su.WAYMO_PALETTE)
    t_sem = (time.perf_counter() - t0) * n / 6
    from infinicube_amd.utils.buffer_utils import generate_coordinate_buffer_from_memory_global_norm as gen
    t_gen = {}
    for mode in ("device", "reference"):
        torch.manual_seed(0)
        gen(d_dev, cam, poses, return_uint8=True, sampling=mode)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gen(d_dev, cam, poses, return_uint8=True, sampling=mode)
        torch.cuda.synchronize()
        t_gen[mode] = time.perf_counter() - t0
    n_valid = int((depth != 0).sum())
    t0 = time.perf_counter()
    torch.randperm(n_valid)
    t_perm = time.perf_counter() - t0
    assert t_gen["device"] < 0.150, f"whole coordinate-buffer function with device sampling: {t_gen['device'] * 1e3:.1f} ms (bar: 150 ms at 93x480x832)"
    lines += ["", f"whole `generate_coordinate_buffer_from_memory_global_norm` (depth resident in HBM, uint8 out): **{t_gen['device'] * 1e3:.1f} ms** with the "
                  f"opt-in device-side sample (stratified pick + device quantile); {t_gen['reference'] * 1e3:.1f} ms with sampling=\"reference\", of which "
                  f"{t_perm * 1e3:.1f} ms is the host `torch.randperm({n_valid})` the reference draws its <=100000-point sample with "
                  f"(kept call for call behind the flag so that a seeded run reproduces the reference's bytes); the three kernels together take < 0.5 ms",
              f"CPU restatement of the reference function (oracle/buffer_ref.py, torch CPU, {torch.get_num_threads()} threads; 6 frames scaled to 93): coordinate buffer {t_coord:.2f} s, semantic_to_color {t_sem:.2f} s"]
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    os.makedirs("gpurun_out", exist_ok=True)
    with open("gpurun_out/buffers_throughput.md", "w") as f:
        f.write("\n".join(lines) + "\n")
