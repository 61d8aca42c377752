"""The voxel ray-cast away from the forward-looking camera, on the CPU: the inputs of tests/voxel_cases.py against the two
oracles of oracle/voxel_ref.py, and against a scalar restatement of the kernel's brick-skipping walk.

(a) ``raycast_dda`` (float32 cell walk, what the kernel must equal bit for bit) against ``raycast_bruteforce`` (float64,
    every voxel against every ray) on every view of the view table, 16 x 12 rays each, scene ``_scene(1, 1500)``.  Bars:
    equal hit indices and |depth difference| < 1e-3 on every non-ambiguous ray (the bars of
    test_voxel_render.py::test_oracle_walk_agrees_with_bruteforce), at most 5 % ambiguous rays PER VIEW.  Measured:

        view               ambiguous   hit mismatches   max |depth diff|   hits / 192
        neg_x_inside         0.00 %          0             1.9e-6             75
        pos_y                0.00 %          0             6.9e-7             37
        neg_y                0.00 %          0             2.0e-6             59
        down_from_4m         0.00 %          0             1.7e-6            111
        up_from_below        2.60 %          0             5.4e-6            192   (all hits: the camera sits under the box)
        outside_far_pos_x    0.00 %          0             3.4e-6             21
        outside_diag_neg     0.00 %          0             3.1e-6             29
        outside_diag_pos     0.52 %          0             3.6e-6             26
        exact_neg_x          0.00 %          0             1.6e-6             69

    (A camera ON the voxel lattice makes brute force call every ray of its centre row or column ambiguous - the ray runs
    along a voxel face - which is why the two vertical cameras stand off the lattice.  The lattice set is not given to
    brute force for the same reason: its ties are exactly what brute force marks ambiguous.)

(b) ``voxel_cases.kernel_walk``, the kernel's walk WITH the brick skip restated in scalar float32, equals ``raycast_dda``
    bit for bit (depth bits and indices) on the view table, on the lattice set and on its anisotropic variant, each
    lattice set at the three eps pairs of ``LATTICE_EPS``.  That is the claim in the kernel's header - the skip lands on
    the cell the cell walk would have reached and changes no float - checked on the inputs where it could fail.

(c) Seven planted mistakes (``voxel_cases.MUTATIONS``) in that restatement: every one changes at least one ray of the new
    sets.  Measured, rays changed (depth bits or index) out of 1728 view rays / 648 lattice rays per eps pair, and out of
    the 576 rays of the old forward-looking poses ``_poses(3)`` at the same 16 x 12 camera:

        mutation   view table   lattice (3 eps pairs)   anisotropic (3 eps pairs)   old poses
        M1            147          18 / 19 / 15            15 / 16 / 11               0   not detected
        M2            283          22 / 23 / 19            17 / 18 / 14               0   not detected
        M3              0           0 /  2 /  0             0 /  1 /  0               0   not detected
        M4              0           0 /  1 /  0             0 /  1 /  0               0   not detected
        M5              0           1 /  0 /  2             2 /  0 /  4               0   not detected
        M6              0          19 / 19 / 11            15 / 15 /  9               0   not detected
        M7              0           4 /  4 /  4             4 /  4 /  4               0   not detected

    new sets: every mutation detected; old poses: none.  For M1 and M2 that is a matter of reading (both sit behind
    ``step[0] < 0``, and every old ray has step[0] == +1); for M3 - M7 it is what these 576 rays happen to show.
    M3 and M4 reorder TIED crossings only: the cells they skip are visited for zero length, so they can start no hit
    and no run that outlasts an eps >= 0.  They are observable through eps < 0 alone (every touched voxel counts), which
    is why the lattice set is also cast with (eps_depth, eps_voxel) = (-1, -1).  M7 is invisible on the view table
    because a walk started at the clamped cell without the clip catches up through the 8 empty padding cells - face
    times are pure functions of the cell - so the lattice volume has no padding.  M5 needs a run not longer than
    eps_depth that ends on a brick face with an empty brick behind it; at 64 x 48 rays the view table has two such rays
    (outside_diag_neg), at 16 x 12 none, and the lattice scene plants some (``TRAP_ORIGIN``).

Regression: ``raycast_dda`` clipped with ``np.maximum(+0., -0.)``, whose sign depends on numpy's loop; a ray that starts
on the volume's far face ((D - o) * inv == -0) then carried t0 = -0 into run_start and flipped the sign of a zero depth.
"""
import functools
import warnings

import numpy as np
import pytest

import voxel_cases as C
from oracle import voxel_ref as V

CANYON_VS = (0.2, 0.2, 0.2)


@functools.lru_cache(maxsize=None)
def _canyon():
    p, s, _ = C._scene(1, 1500)
    ijk, _ = V.points_to_voxels(p, {"semantics": s}, CANYON_VS)
    vol, vmin, dims = V.dense_volume(ijk)
    for a in (ijk, vol, vmin):
        a.setflags(write=False)
    return ijk, vol, vmin


def _cam_rays():
    return C.Cam(16, 12, 12.0).rays.reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def _sets():
    """name -> arguments of raycast_dda / kernel_walk.  "old" is not one of the new sets."""
    _, vol, vmin = _canyon()
    out = {"views": (vol, vmin, CANYON_VS, _cam_rays(), np.stack([C.view_pose(n) for n in C.VIEW_NAMES])),
           "old": (vol, vmin, CANYON_VS, _cam_rays(), C._poses(3))}
    for aniso in (False, True):
        L = C.lattice_case(aniso)
        lv, lmin, _ = V.dense_volume(L["ijk"], pad=L["pad"])
        for eps in C.LATTICE_EPS:
            out[f"{'aniso' if aniso else 'lattice'}-eps{eps[0]:g}"] = (lv, lmin, L["voxel_size"], L["rays"], L["poses"]) + eps
    return out


NEW_SETS = ("views",) + tuple(f"{k}-eps{e[0]:g}" for k in ("lattice", "aniso") for e in C.LATTICE_EPS)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)        # huge face times of the tiny-component rays overflow to inf
        d, h = V.raycast_dda(*_sets()[name])
    d.setflags(write=False), h.setflags(write=False)
    return d, h


def _changed(got, want):
    return (got[0].view(np.int32) != want[0].view(np.int32)) | (got[1] != want[1])


def test_look_follows_the_camera_convention():
    """x right, y down, z forward: looking along +x with z up reproduces ``_poses``'s base rotation exactly."""
    m = C.look((1, 0, 0), (0, 0, 1), (0, 0, 1.6))
    assert np.array_equal(m, C._poses(1)[0] - np.array([[0, 0, 0, 1.0], [0] * 4, [0] * 4, [0] * 4], np.float32))
    m = C.view_pose("exact_neg_x")
    assert np.array_equal(m[:3, :3], np.array([[0, 0, -1], [1, 0, 0], [0, -1, 0]], np.float32))
    for name in C.VIEW_NAMES:
        r = C.view_pose(name)[:3, :3].astype(np.float64)
        assert np.abs(r @ r.T - np.eye(3)).max() < 1e-6 and np.linalg.det(r) > 0.999


def test_view_table_covers_every_step_sign_and_outside_starts():
    """Across the table every axis steps forwards, backwards and not at all; the outside cameras are outside the box."""
    _, vol, vmin = _canyon()
    wd = C.world_directions(_cam_rays(), np.stack([C.view_pose(n) for n in C.VIEW_NAMES]))
    for i in range(3):
        assert (wd[..., i] < 0).any() and (wd[..., i] > 0).any() and (wd[..., i] == 0).any(), f"axis {i}"
    lo = vmin * 0.2
    hi = lo + np.array(vol.shape[::-1]) * 0.2
    for name in C.VIEW_NAMES:
        p = C.view_pose(name)[:3, 3]
        assert bool(((p < lo) | (p > hi)).any()) == (name in C.OUTSIDE_VIEWS), name
    old = C.world_directions(_cam_rays(), C._poses(3))
    assert (old[..., 0] > 0).all()                                   # what the first tests covered


@pytest.mark.parametrize("name", C.VIEW_NAMES)
def test_cell_walk_agrees_with_bruteforce_in_every_view(name):
    ijk, vol, vmin = _canyon()
    k = C.VIEW_NAMES.index(name)
    d, h = (x[k] for x in _oracle("views"))
    db, hb, amb = (x[0] for x in V.raycast_bruteforce(ijk, CANYON_VS, _cam_rays(), C.view_pose(name)[None]))
    ok = ~amb
    err = float(np.abs(d[ok] - db[ok]).max())
    print(f"{name}: ambiguous {amb.mean() * 100:.2f} %, hit mismatches {int((h[ok] != hb[ok]).sum())}, max depth error {err:.2e}, hits {int((h >= 0).sum())}")
    assert amb.mean() <= 0.05
    assert np.array_equal(h[ok], hb[ok]), f"{(h[ok] != hb[ok]).sum()} rays: first voxel differs between the cell walk and brute force"
    assert err < 1e-3
    assert (h >= 0).any() and (d != 0).any()
    if name != "up_from_below":
        assert (h < 0).any() and (d == 0).any()


@pytest.mark.parametrize("name", NEW_SETS + ("old",))
def test_kernel_walk_equals_cell_walk_bit_for_bit(name):
    want = _oracle(name)
    got = C.kernel_walk(*_sets()[name])
    bad = _changed(got, want)
    assert not bad.any(), f"{int(bad.sum())} rays differ; first (pose, ray) = {np.argwhere(bad)[0].tolist()}"
    assert (want[1] >= 0).any() and (want[1] < 0).any()


def test_zero_depth_keeps_its_sign_on_the_far_face():
    """The ray from the volume's high corner along (-1, -1, -1): tb = (D - o) * inv = 0 * negative = -0 on every axis, so
    the clip is fmaxf(+0, -0).  The hardware's max (and C's) order -0 below +0: t0 = +0, the run starts at +0 in the
    occupied corner voxel, and the z-depth is +0 * rz = -0.  (np.maximum returned -0 here, giving +0.)"""
    L = C.lattice_case()
    lv, lmin, _ = V.dense_volume(L["ijk"], pad=0)
    n = int(np.flatnonzero((L["origins_cells"] == C.LATTICE_EXTENT).all(1))[0])
    px = int(np.flatnonzero((L["rays"] < -0.5).all(1))[0])
    corner_voxel = int(np.flatnonzero((L["ijk"] == C.LATTICE_OFFSET + C.LATTICE_EXTENT - 1).all(1))[0])
    d, h = V.raycast_dda(lv, lmin, L["voxel_size"], L["rays"][px:px + 1], L["poses"][n:n + 1])
    assert h[0, 0] == corner_voxel
    assert d[0, 0] == 0 and np.signbit(d[0, 0]), "zero depth times a negative ray z is -0"


OLD_POSES_CANNOT_SEE = ("M1", "M2")          # by reading: both need step[0] < 0


@pytest.mark.parametrize("mutation", list(C.MUTATIONS))
def test_mutation_is_seen_by_the_new_sets(mutation):
    """The planted mistake changes at least one ray of the new sets (the table in the module docstring)."""
    counts = {}
    for name in NEW_SETS:
        counts[name] = int(_changed(C.kernel_walk(*_sets()[name], mutation=mutation), _oracle(name)).sum())
    old = int(_changed(C.kernel_walk(*_sets()["old"], mutation=mutation), _oracle("old")).sum())
    print(f"{mutation} ({C.MUTATIONS[mutation]}): rays changed {counts}; old poses {old}")
    assert sum(counts.values()) > 0, f"{mutation} is invisible to every new set"
    if mutation in OLD_POSES_CANNOT_SEE:
        assert old == 0
        assert counts["views"] > 0
