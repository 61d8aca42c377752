"""Shared inputs of the voxel ray-cast tests (tests/test_voxel_render.py, test_voxel_raycast_cpu.py,
test_voxel_raycast_gpu.py): no test functions.

* ``Cam`` / ``_scene`` / ``_poses``: the street canyon and the forward-looking camera path the first tests were written on.
  Every ray of ``_poses`` has step[0] == +1 and starts inside the volume's box.
* ``look`` and the VIEW TABLE (``VIEWS``): cameras on the same canyon that look along -x, +y, -y, straight down and
  straight up, three cameras outside the volume's box (the clip to the volume, t0 > 0) and one whose forward axis is
  exactly (-1, 0, 0) (its centre column / row has an exactly zero direction component).
* the LATTICE SET (``lattice_case``): voxel size 0.25 (exact in float32, so grid coordinates are exact integers),
  random 5^3 blobs in a volume without padding whose occupied box touches all six faces, identity-rotation poses whose
  origins are cell corners (inside, both corners of the volume, its centre, outside on either side), and every direction
  of {-1, 0, 1}^3 plus four skewed ones.  Face-time ties, brick-corner crossings and the ``o == D`` / ``o == 0`` misses
  live here.  ``anisotropic=True`` is the same set with voxel sizes (0.25, 0.5, 0.125).
* tiny-component rays (``TINY_DIRECTIONS``): direction components that are tiny but NORMAL float32 numbers, so face
  times become huge or overflow to +-inf while every operation stays IEEE-defined.

OUT OF CONTRACT, not tested: a DENORMAL direction component.  ``1 / dg`` then overflows to inf, ``(0 - o) * inf`` is NaN
for ``o == 0``, and the kernel's ``fmaxf`` / ``fminf`` (which drop a NaN operand) differ from ``np.maximum`` /
``np.minimum`` (which propagate it): the kernel and the oracle are not comparable there.  Normalised camera rays times a
rotation do not produce such components short of 1e-38.

* ``kernel_walk``: a scalar-float32 numpy restatement of ``voxel_raycast_kernel`` INCLUDING the brick skip (the oracle
  ``raycast_dda`` is the plain cell walk), operation for operation.  It is the CPU instrument that tells which input
  classes can see which mistake in the skip logic (``MUTATIONS``); it is test infrastructure, not an oracle.
"""
import functools
import math

import numpy as np
import torch

F = np.float32


class Cam:
    def __init__(self, w, h, f):
        self.w, self.h = w, h
        u, v = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
        r = np.stack([(u - w / 2) / f, (v - h / 2) / f, np.ones_like(u)], -1)
        self.rays = (r / np.linalg.norm(r, axis=-1, keepdims=True)).astype(np.float32)

    def get_rays(self):
        return torch.from_numpy(self.rays)


def _scene(seed=0, n_pts=6000):
    """Street canyon point cloud in a z-up world: ground, two walls, a few boxes; camera looks along +x."""
    g = np.random.default_rng(seed)
    ground = np.stack([g.uniform(0, 30, n_pts), g.uniform(-6, 6, n_pts), g.normal(0, 0.02, n_pts)], 1)
    wall_l = np.stack([g.uniform(0, 30, n_pts // 2), np.full(n_pts // 2, 6.0) + g.normal(0, 0.03, n_pts // 2), g.uniform(0, 5, n_pts // 2)], 1)
    wall_r = wall_l * np.array([1, -1, 1])
    box = np.stack([g.uniform(12, 14, 800), g.uniform(-1, 1, 800), g.uniform(0, 1.5, 800)], 1)
    thin = np.stack([np.full(60, 8.03), g.uniform(-0.5, 0.5, 60), g.uniform(0.5, 1.0, 60)], 1)     # a one-voxel-thick sheet (eps cases)
    pts = np.concatenate([ground, wall_l, wall_r, box, thin]).astype(np.float32)
    sem = np.concatenate([np.full(len(ground), 18), np.full(len(wall_l) * 2, 14), np.full(len(box), 1), np.full(len(thin), 10)]).astype(np.int32)
    sem[g.integers(0, len(sem), 200)] = 15                      # label noise: exercises the per-voxel mode
    inst = np.where(sem == 1, 7, 0).astype(np.int32)
    return pts, sem, inst


def _poses(n):
    # camera (x right, y down, z front) -> world (x front, y left, z up), moving forward, slight yaw
    base = np.array([[0, 0, 1, 0], [-1, 0, 0, 0], [0, -1, 0, 1.6], [0, 0, 0, 1]], np.float32)
    out = []
    for i in range(n):
        yaw = 0.05 * i
        rz = np.array([[np.cos(yaw), -np.sin(yaw), 0, 1.0 + 0.7 * i], [np.sin(yaw), np.cos(yaw), 0, 0.1 * i], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)
        out.append(rz @ base)
    return np.stack(out).astype(np.float32)


# ---------------------------------------------------------------------------------------------------
# the view table
# ---------------------------------------------------------------------------------------------------
def look(forward, up, position):
    """4x4 float32 camera-to-world pose of a camera at ``position`` looking along ``forward``: camera x = right,
    y = down, z = forward (the convention of ``_poses``).  Axis-aligned ``forward`` and ``up`` give an exact rotation."""
    f = np.asarray(forward, np.float64)
    f = f / np.linalg.norm(f)
    right = np.cross(f, np.asarray(up, np.float64))
    right = right / np.linalg.norm(right)
    down = np.cross(f, right)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, down, f, np.asarray(position, np.float64)
    return m.astype(np.float32) + np.float32(0)            # + 0: no negative zeros in the matrix


# name -> (forward, up, position).  The canyon spans x 0..30, y -6..6 (walls), z 0..5; with 0.2 m voxels and 8 cells of
# padding the volume's box ends about 1.6 - 3.2 m beyond that on every side, so the three "outside" cameras are outside.
VIEWS = {
    "neg_x_inside": ((-1.0, 0.06, -0.03), (0, 0, 1), (26.0, 0.4, 1.6)),
    "pos_y": ((0.04, 1.0, 0.05), (0, 0, 1), (10.0, -1.0, 1.6)),
    "neg_y": ((-0.05, -1.0, 0.03), (0, 0, 1), (17.0, 1.5, 1.2)),
    "down_from_4m": ((0, 0, -1), (1, 0, 0), (13.13, 0.37, 4.0)),
    "up_from_below": ((0, 0, 1), (1, 0, 0), (12.87, 0.27, -1.0)),
    "outside_far_pos_x": ((-1.0, -0.02, -0.03), (0, 0, 1), (45.0, 1.0, 2.0)),
    "outside_diag_neg": ((-1.0, -0.5, -0.3), (0, 0, 1), (40.0, 14.0, 10.0)),
    "outside_diag_pos": ((1.0, 0.6, 0.25), (0, 0, 1), (-9.0, -13.0, -4.5)),
    "exact_neg_x": ((-1, 0, 0), (0, 0, 1), (20.1, 0.13, 1.7)),
}
VIEW_NAMES = tuple(VIEWS)
OUTSIDE_VIEWS = ("outside_far_pos_x", "outside_diag_neg", "outside_diag_pos")


def view_pose(name):
    return look(*VIEWS[name])


def world_directions(rays_cam, poses):
    """float32 world directions [N, HW, 3] in the kernel's order (products and sums rounded one by one, left to right)."""
    r, m = rays_cam.reshape(-1, 3).astype(F), poses.astype(F)
    return np.stack([((m[:, i, 0][:, None] * r[None, :, 0]) + (m[:, i, 1][:, None] * r[None, :, 1])) + (m[:, i, 2][:, None] * r[None, :, 2])
                     for i in range(3)], -1)


# ---------------------------------------------------------------------------------------------------
# the lattice set
# ---------------------------------------------------------------------------------------------------
LATTICE_VS, ANISO_VS = (0.25, 0.25, 0.25), (0.25, 0.5, 0.125)
LATTICE_EXTENT = np.array([80, 64, 40])            # cells; 10 x 8 x 5 bricks
LATTICE_OFFSET = np.array([-16, 8, -8])            # ijk of cell (0, 0, 0): multiples of 8, so no padding is added at pad = 0
TRAP_ORIGIN = np.array([24, 24, 8])                # a brick corner; lattice_case plants voxels along the axes through it
LATTICE_EPS = ((1e-1, 1e-2), (-1.0, -1.0), (0.3, 0.3))   # (eps_depth, eps_voxel): the defaults; every touched voxel counts, zero-length
#                                                          visits included (the ORDER of tied crossings shows); more than one voxel
SKEW_DIRECTIONS = ((1, 2, 0), (-2, 1, 1), (3, -1, 2), (-1, -2, -3))
TINY_DIRECTIONS = ((1e-20, 1, 0), (1, -1e-20, 1e-20), (-1e-20, -1e-20, 1), (0, 3e-38, -1), (-3e-38, 1, 3e-38), (1, 1, 1e-30))


def lattice_directions():
    """[30 + 6, 3] float32: {-1, 0, 1}^3 without 0, the skewed four, the tiny-component six; each v / |v|, so the equal
    components of a diagonal are the same float and (1, 2, 0) keeps its exact 1 : 2 ratio."""
    cube = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]
    v = np.array(cube + list(SKEW_DIRECTIONS) + list(TINY_DIRECTIONS), np.float64)
    out = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)
    assert (np.abs(out[out != 0]) >= np.finfo(F).tiny).all(), "a denormal component is out of contract"
    return out


@functools.lru_cache(maxsize=None)
def lattice_case(anisotropic=False):
    """-> dict(ijk, sem, voxel_size, pad=0, rays [HW, 3], poses [N, 4, 4], origins_cells [N, 3]).  About 40 random 5^3
    blobs in an 80 x 64 x 40 volume (most of the 400 bricks stay empty), one blob pinned into each extreme corner so that
    occupied cells lie ON the volume's faces (a ray that ought to miss there, and does not, hits something)."""
    g = np.random.default_rng(11)
    E = LATTICE_EXTENT
    lows = [np.zeros(3, np.int64), E - 5] + [g.integers(0, E - 4) for _ in range(38)]
    lows += [np.array([19, 27, 11]), np.array([35, 11, 27])]           # two blobs whose high faces lie on brick faces
    cells = np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(5), indexing="ij"), -1).reshape(-1, 3)
    # single voxels that END a brick along +-x, +-y, +z as seen from TRAP_ORIGIN, an empty stretch, then a 3-voxel run: with
    # eps_depth above one voxel the single voxel's run must be dropped when the ray enters the empty brick behind it
    traps = [TRAP_ORIGIN + np.array(t) for t in ((7, 0, 0), (20, 0, 0), (21, 0, 0), (22, 0, 0), (-8, 0, 0), (-14, 0, 0), (-15, 0, 0), (-16, 0, 0),
                                                  (0, 7, 0), (0, 20, 0), (0, 21, 0), (0, 22, 0), (0, -8, 0), (0, -14, 0), (0, -15, 0), (0, -16, 0),
                                                  (0, 0, 7), (0, 0, 20), (0, 0, 21), (0, 0, 22))]
    ijk = np.unique(np.concatenate([lo + cells for lo in lows] + [np.stack(traps)]), axis=0)
    ijk = ijk[np.lexsort((ijk[:, 0], ijk[:, 1], ijk[:, 2]))] + LATTICE_OFFSET
    sem = ((ijk[:, 0] * 7 + ijk[:, 1] * 3 + ijk[:, 2]) % 19 + 1).astype(np.int32)
    vs = np.array(ANISO_VS if anisotropic else LATTICE_VS, np.float64)
    inside = [g.integers(1, E) for _ in range(8)] + [8 * g.integers(1, E // 8) for _ in range(4)]      # the last four: brick corners
    corners = np.array(inside + [np.zeros(3, np.int64), E, E // 2, np.full(3, -3), E + 8, TRAP_ORIGIN])
    poses = np.tile(np.eye(4, dtype=F), (len(corners), 1, 1))
    world = (corners + LATTICE_OFFSET) * vs                             # exact: multiples of 1/8
    poses[:, :3, 3] = world.astype(F)
    assert np.array_equal(poses[:, :3, 3].astype(np.float64), world)
    out = dict(ijk=ijk.astype(np.int32), sem=sem, voxel_size=tuple(float(x) for x in vs), pad=0, rays=lattice_directions(),
               poses=poses, origins_cells=corners)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------
# scalar float32 restatement of voxel_raycast_kernel (csrc/voxels.hip), brick skip included
# ---------------------------------------------------------------------------------------------------
MUTATIONS = {
    "M1": "exit cell on a negative step of axis 0 is bb instead of bb - 1",
    "M2": "brick face on a negative step of axis 0 uses the +1 brick",
    "M3": "the tie rule `tf == ts && i < a` is loosened to `tf == ts`",
    "M4": "the brick-axis choice uses <=",
    "M5": "the skip branch does not close an open run",
    "M6": "the zero-step miss test is removed",
    "M7": "the t0 clip is ignored",
}
_INF, _ZERO, _ONE = F(np.inf), F(0.0), F(1.0)


def brick_map(vol):
    Dz, Dy, Dx = vol.shape
    return (vol.reshape(Dz // 8, 8, Dy // 8, 8, Dx // 8, 8) >= 0).any(axis=(1, 3, 5))


def kernel_walk(vol, vol_min, voxel_size, rays_cam, poses, eps_depth=1e-1, eps_voxel=1e-2, mutation=None):
    """-> (zdepth f32 [N, HW], hit i32 [N, HW]) like ``oracle.voxel_ref.raycast_dda``, computed the way the kernel does:
    one ray at a time, np.float32 scalars (every operation rounds to float32, no contraction), the same comparisons in
    the same order, empty 8^3 bricks skipped.  ``mutation`` (a key of MUTATIONS) plants one mistake.

    The kernel's loop guard is 2^20 iterations; the walk proper needs at most Dx + Dy + Dz.  Here the guard is
    4 (Dx + Dy + Dz) + 64, and a skip that leaves (c, t_cur) where they were ends the walk at once: a mutated walk that
    stops advancing keeps its whole state fixed, so where it is cut makes no difference to its result.  The unmutated
    walk must reach neither (asserted)."""
    assert mutation is None or mutation in MUTATIONS
    mut = mutation
    vs = np.asarray(voxel_size, F)
    Dz, Dy, Dx = vol.shape
    D = (Dx, Dy, Dz)
    bricks = brick_map(vol)
    g = (np.asarray(vol_min).astype(np.float64) * vs.astype(np.float64)).astype(F)      # grid_lo3 as VoxelVolume.raycast passes it
    iv = [_ONE / vs[i] for i in range(3)]                                              # p.ivx = 1.0f / voxel_size3[0]
    r = np.asarray(rays_cam, F).reshape(-1, 3)
    P = np.asarray(poses, F)
    N, HW = P.shape[0], r.shape[0]
    out_d, out_h = np.zeros((N, HW), F), np.full((N, HW), -1, np.int32)
    ed, ev = F(eps_depth), F(eps_voxel)
    guard_max = 4 * (Dx + Dy + Dz) + 64

    def face_time(o, inv, step, c):
        return _INF if step == 0 else (F(c + 1 if step > 0 else c) - o) * inv

    with np.errstate(all="ignore"):
        for n in range(N):
            m = P[n]
            for pix in range(HW):
                rx, ry, rz = r[pix]
                d, o, inv, step = [None] * 3, [None] * 3, [None] * 3, [0] * 3
                for i in range(3):
                    d[i] = ((m[i, 0] * rx) + (m[i, 1] * ry)) + (m[i, 2] * rz)
                for i in range(3):
                    o[i] = (m[i, 3] - g[i]) * iv[i]
                    dg = d[i] * iv[i]
                    step[i] = 1 if dg > _ZERO else (-1 if dg < _ZERO else 0)
                    inv[i] = _ONE / dg if step[i] else _ZERO
                    d[i] = dg
                t0, t1, miss = _ZERO, _INF, False
                for i in range(3):
                    if step[i] == 0:
                        if mut != "M6" and (o[i] < _ZERO or o[i] >= F(D[i])):
                            miss = True
                    else:
                        ta, tb = (_ZERO - o[i]) * inv[i], (F(D[i]) - o[i]) * inv[i]
                        lo, hi = (ta if ta <= tb else tb), (ta if ta >= tb else tb)
                        if mut != "M7":
                            t0 = t0 if t0 >= lo else lo
                        t1 = t1 if t1 <= hi else hi
                depth, hit = _ZERO, -1
                if not miss and t0 < t1:
                    c = [0] * 3
                    for i in range(3):
                        ci = math.floor(o[i] + t0 * d[i])
                        c[i] = 0 if ci < 0 else (D[i] - 1 if ci >= D[i] else ci)
                    t_cur, run_start = t0, _ZERO
                    in_run = depth_done = hit_done = False
                    guard = 0
                    while guard < guard_max:
                        guard += 1
                        if c[0] < 0 or c[1] < 0 or c[2] < 0 or c[0] >= Dx or c[1] >= Dy or c[2] >= Dz:
                            break
                        if not bricks[c[2] >> 3, c[1] >> 3, c[0] >> 3]:
                            if in_run and mut != "M5":
                                in_run = False
                                if not depth_done and t_cur - run_start > ed:
                                    depth, depth_done = run_start, True
                            if depth_done and hit_done:
                                break
                            tb3, bb = [None] * 3, [0] * 3
                            for i in range(3):
                                up = step[i] > 0 or (mut == "M2" and i == 0 and step[i] < 0)
                                bb[i] = ((c[i] >> 3) + 1) << 3 if up else (c[i] >> 3) << 3
                                tb3[i] = _INF if step[i] == 0 else (F(bb[i]) - o[i]) * inv[i]
                            a = 0
                            if mut == "M4":
                                if tb3[1] <= tb3[a]:
                                    a = 1
                                if tb3[2] <= tb3[a]:
                                    a = 2
                            else:
                                if tb3[1] < tb3[a]:
                                    a = 1
                                if tb3[2] < tb3[a]:
                                    a = 2
                            ts = tb3[a]
                            for i in range(3):
                                if i == a or step[i] == 0:
                                    continue
                                for _ in range(8):
                                    tf = face_time(o[i], inv[i], step[i], c[i])
                                    if tf < ts or (tf == ts and (i < a or mut == "M3")):
                                        c[i] += step[i]
                                    else:
                                        break
                            before = (c[0], c[1], c[2], t_cur)
                            if step[a] > 0 or (mut == "M1" and a == 0):
                                c[a] = bb[a]
                            else:
                                c[a] = bb[a] - 1
                            t_cur = ts
                            if before == (c[0], c[1], c[2], t_cur):
                                assert mut is not None
                                break                       # a mutated skip that goes nowhere: the kernel would spin to its guard on this state
                            continue
                        idx = int(vol[c[2], c[1], c[0]])
                        a, t_out = 0, face_time(o[0], inv[0], step[0], c[0])
                        ty = face_time(o[1], inv[1], step[1], c[1])
                        tz = face_time(o[2], inv[2], step[2], c[2])
                        if ty < t_out:
                            a, t_out = 1, ty
                        if tz < t_out:
                            a, t_out = 2, tz
                        if idx >= 0:
                            if not hit_done and t_out - t_cur > ev:
                                hit, hit_done = idx, True
                            if not in_run:
                                in_run, run_start = True, t_cur
                        elif in_run:
                            in_run = False
                            if not depth_done and t_cur - run_start > ed:
                                depth, depth_done = run_start, True
                        if depth_done and hit_done:
                            break
                        c[a] += step[a]
                        t_cur = t_out
                    else:
                        assert mut is not None, "the unmutated walk ran into its guard"
                    if in_run and not depth_done and t_cur - run_start > ed:
                        depth = run_start
                out_d[n, pix] = depth * rz
                out_h[n, pix] = hit
    return out_d, out_h
