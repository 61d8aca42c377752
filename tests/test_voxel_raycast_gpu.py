"""csrc/voxels.hip on the inputs of tests/voxel_cases.py: rays in every octant, cameras outside the volume, exact face-time
ties, tiny direction components, every output selection of the C ABI, the scatter kernel's box test, per-frame rendering
and the eps comparisons.  Every kernel comparison is ``np.array_equal`` against ``oracle.voxel_ref.raycast_dda`` on the
same voxel list: depth as float32 BITS, hit indices as integers.  No tolerance anywhere.

tests/test_voxel_raycast_cpu.py shows on a CPU restatement of the kernel which of these inputs see which mistake; what
this pins is the compiled kernel to the oracle's cell walk.  It does not pin the oracle to fVDB (ORACLE_RISKS.md R26).
"""
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

import voxel_cases as C
from oracle import voxel_ref as V

VS = (0.2, 0.2, 0.2)
SENTINEL = 0x5A5AA5A5          # one int32 word; no voxel index, class, background or depth of these tests has these bits
GUARD_WORDS = 64


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _dda(*args, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)        # huge face times of the tiny-component rays overflow to inf
        return V.raycast_dda(*args, **kw)


@functools.lru_cache(maxsize=None)
def _canyon():
    """The canyon of test_voxel_render.py (seed 2, 6000 points per surface), voxelised by the product code on the GPU;
    the dense volume the oracle walks is built from the SAME voxel list.  Built once for every test of this module."""
    from infinicube_amd.utils.voxel_render import VoxelVolume, points_to_voxels
    p, s, i = C._scene(2)
    ijk, attrs = points_to_voxels(torch.from_numpy(p).cuda(), {"semantics": torch.from_numpy(s).cuda(), "instance": torch.from_numpy(i).cuda()})
    volume = VoxelVolume.build(ijk)
    vol, vmin, dims = V.dense_volume(ijk.cpu().numpy())
    assert np.array_equal(vmin, volume.vol_min) and np.array_equal(dims, volume.dims) and np.array_equal(vol, volume.vol.cpu().numpy())
    assert np.array_equal(volume.bricks.cpu().numpy().astype(bool), C.brick_map(vol))
    vol.setflags(write=False)
    return volume, attrs, vol, vmin


@functools.lru_cache(maxsize=None)
def _table_steps():
    """Signs of the world direction components over the whole view table at the 64 x 48 camera: [9, 3072, 3]."""
    return np.sign(C.world_directions(C.Cam(64, 48, 50.0).rays, np.stack([C.view_pose(n) for n in C.VIEW_NAMES])))


@pytest.mark.gpu
@pytest.mark.parametrize("name", C.VIEW_NAMES)
def test_raycast_every_view_bit_exact(name):
    volume, attrs, vol, vmin = _canyon()
    st = _table_steps()
    for axis in range(3):          # the table as a whole drives every axis forwards, backwards and not at all
        assert (st[..., axis] < 0).any() and (st[..., axis] > 0).any() and (st[..., axis] == 0).any(), f"axis {axis}"
    cam = C.Cam(64, 48, 50.0)
    pose = C.view_pose(name)[None]
    depth, sem, inst, idx = volume.raycast(cam.get_rays(), torch.from_numpy(pose), attrs["semantics"], attrs["instance"], want_index=True)
    d, h = _dda(vol, vmin, VS, cam.rays.reshape(-1, 3), pose)
    got_h = idx.cpu().numpy().reshape(1, -1)
    assert (h >= 0).any() and (d != 0).any()
    if name != "up_from_below":
        assert (h < 0).any()
    assert np.array_equal(got_h, h), f"{(got_h != h).sum()} rays hit a different voxel than the oracle's cell walk"
    got_d = depth.cpu().numpy().reshape(1, -1)
    assert np.array_equal(_bits(got_d), _bits(d)), f"{(_bits(got_d) != _bits(d)).sum()} z-depths differ from the oracle in their bits"
    for got, a in ((sem, attrs["semantics"]), (inst, attrs["instance"])):
        a = a.cpu().numpy()
        assert np.array_equal(got.cpu().numpy().reshape(1, -1), np.where(h >= 0, a[np.maximum(h, 0)], 0))


@pytest.mark.gpu
@pytest.mark.parametrize("anisotropic", [False, True], ids=["cubic", "anisotropic"])
def test_raycast_lattice_ties_bit_exact(anisotropic):
    """Origins on cell corners, all 26 lattice directions, four skewed ones and the tiny-component rays, in a volume
    without padding; each eps pair of LATTICE_EPS ((-1, -1) makes the order of tied crossings visible)."""
    from infinicube_amd.utils.voxel_render import VoxelVolume
    L = C.lattice_case(anisotropic)
    volume = VoxelVolume.build(torch.from_numpy(L["ijk"].copy()), L["voxel_size"], pad=L["pad"])
    vol, vmin, dims = V.dense_volume(L["ijk"], pad=L["pad"])
    assert np.array_equal(vmin, C.LATTICE_OFFSET) and np.array_equal(dims, C.LATTICE_EXTENT)
    assert np.array_equal(vmin, volume.vol_min) and np.array_equal(dims, volume.dims) and np.array_equal(vol, volume.vol.cpu().numpy())
    assert np.array_equal(volume.bricks.cpu().numpy().astype(bool), C.brick_map(vol))
    # the oracle's rule for the low corner, float32(float64(vol_min) * float64(voxel size)), is EXACT here: every origin
    # of this set is an exact integer in grid coordinates, which is what puts the rays on cell corners
    vs32 = np.asarray(L["voxel_size"], np.float32)
    assert np.array_equal(volume.voxel_sizes, vs32)
    glo = (vmin.astype(np.float64) * vs32.astype(np.float64)).astype(np.float32)
    assert np.array_equal(glo.astype(np.float64), vmin * np.asarray(L["voxel_size"]))
    o = (L["poses"][:, :3, 3] - glo) * (np.float32(1) / vs32)
    assert np.array_equal(o, L["origins_cells"].astype(np.float32))
    tiny = np.abs(L["rays"]) < 1e-10
    assert (tiny & (L["rays"] != 0)).any(1).sum() == len(C.TINY_DIRECTIONS)
    sem = torch.from_numpy(L["sem"].copy())
    rays = torch.from_numpy(L["rays"].copy()).reshape(1, -1, 3)
    for eps_depth, eps_voxel in C.LATTICE_EPS:
        depth, s, _, idx = volume.raycast(rays, torch.from_numpy(L["poses"].copy()), sem, None, background0=-3,
                                          eps_depth=eps_depth, eps_voxel=eps_voxel, want_index=True)
        d, h = _dda(vol, vmin, L["voxel_size"], L["rays"], L["poses"], eps_depth, eps_voxel)
        n = len(L["poses"])
        got_h, got_d = idx.cpu().numpy().reshape(n, -1), depth.cpu().numpy().reshape(n, -1)
        assert (h >= 0).sum() >= 30 and (h < 0).sum() >= 30          # the set is neither all hits nor all misses (the oracle's own counts: 37 - 87 hits)
        bad = got_h != h
        assert not bad.any(), f"eps {eps_depth, eps_voxel}: {bad.sum()} hits differ; first (origin, direction) {np.argwhere(bad)[0]}"
        bad = _bits(got_d) != _bits(d)
        assert not bad.any(), f"eps {eps_depth, eps_voxel}: {bad.sum()} depths differ in their bits; first (origin, direction) {np.argwhere(bad)[0]}"
        assert np.array_equal(s.cpu().numpy().reshape(n, -1), np.where(h >= 0, L["sem"][np.maximum(h, 0)], -3))


class Guarded:
    """A device buffer of ``n`` 32-bit words with GUARD_WORDS sentinel words on both sides; the payload starts out as
    sentinel words too, so a word the launch never wrote shows."""

    def __init__(self, n):
        self.n = n
        self.t = torch.full((n + 2 * GUARD_WORDS,), SENTINEL, dtype=torch.int32, device="cuda:0")
        self.ptr = self.t.data_ptr() + 4 * GUARD_WORDS

    def read(self):
        a = self.t.cpu().numpy()
        assert (a[:GUARD_WORDS] == SENTINEL).all() and (a[GUARD_WORDS + self.n:] == SENTINEL).all(), "a guard word was overwritten"
        return a[GUARD_WORDS:GUARD_WORDS + self.n].copy()

    def untouched(self):
        return bool((self.t == SENTINEL).all())


OUTPUTS = ("depth", "attr0", "attr1", "index")


@pytest.mark.gpu
@pytest.mark.parametrize("n_poses,hw", [(1, 1), (1, 255), (1, 257), (3, 1001)], ids=["1", "255", "257", "3x1001"])
def test_raycast_outputs_and_backgrounds(n_poses, hw):
    """icv_voxel_raycast through the C ABI: ray counts off the 256-thread block, backgrounds 255 / -7, a NULL attribute
    table, each output NULL in turn (the others keep their bits), and all four NULL (an error that writes nothing)."""
    from infinicube_amd import native
    lib = native.lib()
    volume, attrs, vol, vmin = _canyon()
    stream = torch.cuda.current_stream().cuda_stream
    all_rays = C.Cam(64, 48, 50.0).rays.reshape(-1, 3)
    rays = all_rays[[48 * 32 + 32]] if hw == 1 else all_rays[np.linspace(0, len(all_rays) - 1, hw).astype(np.int64)]
    poses = np.stack([C.view_pose(n) for n in ("exact_neg_x", "down_from_4m", "outside_diag_neg")][:n_poses])
    d, h = _dda(vol, vmin, VS, rays, poses)
    sem, inst = attrs["semantics"].cpu().numpy(), attrs["instance"].cpu().numpy()
    if hw > 1:
        assert (h >= 0).any() and (h < 0).any()
    want = {"depth": _bits(d).reshape(-1), "index": h.reshape(-1).astype(np.int32),
            "attr0": np.where(h >= 0, sem[np.maximum(h, 0)], 255).reshape(-1), "attr1": np.where(h >= 0, inst[np.maximum(h, 0)], -7).reshape(-1)}
    rays_d, poses_d = torch.from_numpy(rays.copy()).cuda(), torch.from_numpy(poses.reshape(-1, 16).copy()).cuda()
    c3 = lambda a: (ctypes.c_int * 3)(*[int(x) for x in a])       # noqa: E731
    f3 = lambda a: (ctypes.c_float * 3)(*[float(x) for x in a])   # noqa: E731
    glo = (vmin.astype(np.float64) * np.asarray(VS, np.float32).astype(np.float64)).astype(np.float32)

    def launch(selected, attr0=attrs["semantics"], attr1=attrs["instance"]):
        bufs = {k: Guarded(n_poses * hw) for k in OUTPUTS}
        rc = lib.icv_voxel_raycast(volume.vol.data_ptr(), volume.bricks.data_ptr(), c3(volume.dims), f3(glo), f3(volume.voxel_sizes),
                                   rays_d.data_ptr(), poses_d.data_ptr(), n_poses, hw, 0.1, 0.01, native.ptr(attr0), native.ptr(attr1), 255, -7,
                                   *[bufs[k].ptr if k in selected else None for k in OUTPUTS], stream)
        torch.cuda.synchronize()
        return rc, bufs

    rc, full = launch(OUTPUTS)
    assert rc == 0, lib.icv_last_error()
    full = {k: b.read() for k, b in full.items()}
    for k in OUTPUTS:
        assert np.array_equal(full[k], want[k]), f"{k}: {(full[k] != want[k]).sum()} of {n_poses * hw} words differ from the oracle"
    for dropped in OUTPUTS:
        rc, bufs = launch([k for k in OUTPUTS if k != dropped])
        assert rc == 0, lib.icv_last_error()
        assert bufs[dropped].untouched(), f"{dropped} was NULL, yet its buffer was written"
        for k in OUTPUTS:
            if k != dropped:
                assert np.array_equal(bufs[k].read(), full[k]), f"{k} changed when {dropped} was NULL"
    rc, bufs = launch(())
    assert rc != 0 and b"no output" in lib.icv_last_error()
    assert all(b.untouched() for b in bufs.values())
    # attr0 NULL with attr1 given: the attr0 map is the background everywhere, the rest is unchanged
    rc, bufs = launch(OUTPUTS, attr0=None)
    assert rc == 0, lib.icv_last_error()
    assert (bufs["attr0"].read() == 255).all()
    for k in ("depth", "attr1", "index"):
        assert np.array_equal(bufs[k].read(), full[k])
    # both tables NULL, only the index wanted
    rc, bufs = launch(("index",), attr0=None, attr1=None)
    assert rc == 0, lib.icv_last_error()
    assert np.array_equal(bufs["index"].read(), full["index"]) and all(bufs[k].untouched() for k in ("depth", "attr0", "attr1"))


@pytest.mark.gpu
def test_scatter_drops_out_of_box_and_marks_bricks():
    """icv_voxel_scatter with a box smaller than the voxel list: voxels one cell (and many cells) outside each of the six
    faces are dropped, voxels ON the last cell of each axis are kept, the brick map is the any-reduction of the volume."""
    from infinicube_amd import native
    lib = native.lib()
    stream = torch.cuda.current_stream().cuda_stream
    vmin, dims = np.array([-8, 16, 8]), np.array([24, 16, 8])
    hi = vmin + dims
    g = np.random.default_rng(5)
    inside = np.stack([g.integers(vmin[i], hi[i], 800) for i in range(3)], 1)
    inside = inside[(inside[:, 0] < 0) | (inside[:, 0] >= 8) | (inside[:, 1] >= 24)]          # leaves the brick x 0..7, y 16..23 empty
    edge = [vmin, hi - 1, [hi[0] - 1, vmin[1], vmin[2]], [vmin[0], hi[1] - 1, vmin[2]], [vmin[0], vmin[1], hi[2] - 1]]
    outside = []
    for axis in range(3):
        for v in (vmin[axis] - 1, vmin[axis] - 9, hi[axis], hi[axis] + 30):
            for _ in range(3):
                p = np.array([g.integers(vmin[i], hi[i]) for i in range(3)])
                p[axis] = v
                outside.append(p)
    outside.append(vmin - 1)
    outside.append(hi)
    ijk = np.unique(np.concatenate([inside, np.array(edge), np.array(outside)]), axis=0)
    ijk = ijk[g.permutation(len(ijk))].astype(np.int32)                                        # unsorted: the index is the list position
    M = len(ijk)
    assert M % 256 != 0 and M > 512
    in_box = ((ijk >= vmin) & (ijk < hi)).all(1)
    assert 0 < (~in_box).sum() and all(((ijk[:, a] < vmin[a]).any() and (ijk[:, a] >= hi[a]).any()) for a in range(3))
    full, flo, fdims = V.dense_volume(ijk)                                                    # the oracle's volume over the WHOLE list
    off = vmin - flo
    assert (off >= 0).all() and (off + dims <= fdims).all()
    want = full[off[2]:off[2] + dims[2], off[1]:off[1] + dims[1], off[0]:off[0] + dims[0]]
    assert np.array_equal(np.sort(want[want >= 0]), np.flatnonzero(in_box))
    want_bricks = C.brick_map(want)
    assert want_bricks.any() and not want_bricks.all()

    n_vol, n_br = int(dims.prod()), int(dims.prod()) // 512
    guard = 256
    c3 = lambda a: (ctypes.c_int * 3)(*[int(x) for x in a])       # noqa: E731

    def buffers():
        vol = torch.full((n_vol + 2 * GUARD_WORDS,), SENTINEL, dtype=torch.int32, device="cuda:0")
        vol[GUARD_WORDS:GUARD_WORDS + n_vol] = -1
        br = torch.full((n_br + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda:0")
        br[guard:guard + n_br] = 0
        return vol, br

    ijk_d = torch.from_numpy(ijk).cuda()
    vol, br = buffers()
    rc = lib.icv_voxel_scatter(ijk_d.data_ptr(), M, c3(vmin), c3(dims), vol.data_ptr() + 4 * GUARD_WORDS, br.data_ptr() + guard, stream)
    torch.cuda.synchronize()
    assert rc == 0, lib.icv_last_error()
    v, b = vol.cpu().numpy(), br.cpu().numpy()
    assert (v[:GUARD_WORDS] == SENTINEL).all() and (v[GUARD_WORDS + n_vol:] == SENTINEL).all(), "guard words around the volume overwritten"
    assert (b[:guard] == 0xA5).all() and (b[guard + n_br:] == 0xA5).all(), "guard bytes around the brick map overwritten"
    got = v[GUARD_WORDS:GUARD_WORDS + n_vol].reshape(dims[2], dims[1], dims[0])
    got_bricks = b[guard:guard + n_br].reshape(dims[2] // 8, dims[1] // 8, dims[0] // 8)
    assert np.array_equal(got, want), f"{(got != want).sum()} cells differ from the oracle's volume cropped to the box"
    assert set(np.unique(got_bricks)) <= {0, 1}
    assert np.array_equal(got_bricks.astype(bool), want_bricks) and np.array_equal(got_bricks.astype(bool), C.brick_map(got))
    # dims that are no multiples of 8 are refused and nothing is written
    for bad_dims in ([20, 16, 8], [24, 12, 8], [24, 16, 7]):
        vol, br = buffers()
        before_v, before_b = vol.clone(), br.clone()
        rc = lib.icv_voxel_scatter(ijk_d.data_ptr(), M, c3(vmin), c3(bad_dims), vol.data_ptr() + 4 * GUARD_WORDS, br.data_ptr() + guard, stream)
        torch.cuda.synchronize()
        assert rc != 0 and b"multiples of 8" in lib.icv_last_error()
        assert torch.equal(vol, before_v) and torch.equal(br, before_b)


@pytest.mark.gpu
def test_render_frames_equals_per_frame_calls():
    """Two frames with their own point sets (the second carries a moving object's box) and their own poses: render_frames
    equals render_voxel_buffers frame by frame, and each frame equals the oracle on its own voxelisation."""
    from infinicube_amd.utils.voxel_render import render_frames, render_voxel_buffers
    p, s, i = C._scene(4, 1500)
    g = np.random.default_rng(9)
    car = np.stack([g.uniform(5.0, 7.0, 1500), g.uniform(-2.0, -0.5, 1500), g.uniform(0.0, 1.4, 1500)], 1).astype(np.float32)
    pts = [p, np.concatenate([p, car])]
    sems = [s, np.concatenate([s, np.full(len(car), 13, np.int32)])]
    insts = [i, np.concatenate([i, np.full(len(car), 42, np.int32)])]
    poses = np.stack([C._poses(1)[0], C.view_pose("neg_x_inside")])
    poses[1, :3, 3] = (18.0, -0.8, 1.5)
    cam = C.Cam(48, 32, 30.0)
    t = torch.from_numpy
    depth, sem, inst = render_frames(cam, t(poses), [t(x) for x in pts], [t(x) for x in sems], [t(x) for x in insts])
    assert depth.shape == (2, 32, 48) and depth.dtype == torch.float32 and sem.dtype == torch.int32 and inst.dtype == torch.int32
    for f in range(2):
        one = render_voxel_buffers(cam, t(poses[f]), t(pts[f]), t(sems[f]), t(insts[f]))
        for got, ref in zip((depth, sem, inst), one):
            assert np.array_equal(_bits(got[f].cpu().numpy()), _bits(ref.cpu().numpy()))
        ijk, attrs = V.points_to_voxels(pts[f], {"semantics": sems[f], "instance": insts[f]}, VS)
        vol, vmin, _ = V.dense_volume(ijk)
        d, h = _dda(vol, vmin, VS, cam.rays.reshape(-1, 3), poses[f:f + 1])
        assert (h >= 0).any() and (h < 0).any()
        assert np.array_equal(_bits(depth[f].cpu().numpy().reshape(1, -1)), _bits(d))
        assert np.array_equal(sem[f].cpu().numpy().reshape(1, -1), np.where(h >= 0, attrs["semantics"][np.maximum(h, 0)], 0))
        assert np.array_equal(inst[f].cpu().numpy().reshape(1, -1), np.where(h >= 0, attrs["instance"][np.maximum(h, 0)], 0))
    assert not (sem[0] == 13).any() and (sem[1] == 13).any() and (inst[1] == 42).any()        # the object is in frame 1 only


@pytest.mark.gpu
def test_raycast_eps_boundaries():
    """(eps_depth, eps_voxel) = (0, 0); (0.2, 0.2) = exactly one voxel, where the `>` comparisons sit on their boundary
    for axis-parallel crossings; (1.0, 0.3).  The sheet at x = 8.03 is one voxel thick and seen nearly head-on, so no ray
    stays inside one of its voxels for 0.3 m: its class leaves the semantic map at eps_voxel = 0.3."""
    volume, attrs, vol, vmin = _canyon()
    cam = C.Cam(64, 48, 50.0)
    poses = np.stack([C._poses(1)[0], C.view_pose("exact_neg_x")])
    poses[1, :3, 3] = (11.03, 0.1, 0.9)                             # looks back at the sheet along exactly -x
    sa = attrs["semantics"].cpu().numpy()
    seen = {}
    for eps_depth, eps_voxel in ((0.0, 0.0), (0.2, 0.2), (1.0, 0.3)):
        depth, sem, _, idx = volume.raycast(cam.get_rays(), torch.from_numpy(poses), attrs["semantics"], None,
                                            eps_depth=eps_depth, eps_voxel=eps_voxel, want_index=True)
        d, h = _dda(vol, vmin, VS, cam.rays.reshape(-1, 3), poses, eps_depth, eps_voxel)
        got_h, got_d = idx.cpu().numpy().reshape(2, -1), depth.cpu().numpy().reshape(2, -1)
        assert np.array_equal(got_h, h), f"eps {eps_depth, eps_voxel}: {(got_h != h).sum()} hits differ"
        assert np.array_equal(_bits(got_d), _bits(d)), f"eps {eps_depth, eps_voxel}: {(_bits(got_d) != _bits(d)).sum()} depths differ"
        got_s = sem.cpu().numpy().reshape(2, -1)
        assert np.array_equal(got_s, np.where(h >= 0, sa[np.maximum(h, 0)], 0))
        seen[eps_voxel] = [bool((got_s[f] == 10).any()) for f in range(2)]
        assert (d != 0).any() and ((h >= 0).any() or eps_voxel == 0.3)      # no 0.2 m voxel of these views is crossed for 0.3 m
    assert seen[0.0] == [True, True] and seen[0.3] == [False, False], seen
