"""The five guidance-buffer kernels of csrc/buffers.hip away from the shapes tests/test_buffers.py uses: row widths and
pixel counts that are no multiple of 4 (the scalar tails), rows wider than one 1024-pixel block, device pointers that
are not 16- / 4-byte aligned (each term of the kernels' ``vec`` predicate on its own), every output selection, the
global-memory class table and the class clamp of the semantic kernel, instance ids >= 65536, has_valid == 0 on
non-zero depth, and the gathered sample points.

Expected values are the reference's own golden arrays where a crop of them applies, and otherwise the float32 numpy
restatement in oracle/buffer_ref.py, which the first (CPU) test pins to those golden arrays bit for bit.  Every
comparison is ``np.array_equal``; the only tolerances are the two "another host's LAPACK" bars tests/test_buffers.py
already uses, at the wrapper level.  Every device buffer is carved out of one sentinel-filled allocation (``Arena``),
so a store past either end of an output, or into an input, fails the test."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from oracle import buffer_ref as B

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "coord_buffer_cases.npz"))
CASES = ("small", "allsky", "big")
SENTINEL = 0xA5
GUARD = 256          # bytes on both sides of every carved buffer (>= 64, a multiple of 16)


def _host(name):
    return (G[f"{name}_kinv"], G[f"{name}_to_cam0"], G[f"{name}_mins"], G[f"{name}_ranges"], int(G[f"{name}_has_valid"][0]))


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_reference_golden(name):
    """oracle.buffer_ref's float32 restatement of the kernels' arithmetic, fed the host numbers stored beside the golden
    arrays, equals the reference's float32 buffer and the caller's uint8 buffer exactly: its authority for other shapes."""
    kinv, tf, mins, ranges, hv = _host(name)
    f32 = B.coord_normalize_f32(G[f"{name}_depth"], kinv, tf, mins, ranges, hv)
    assert f32.dtype == np.float32 and np.array_equal(f32, G[f"{name}_coord"])
    assert np.array_equal(B.coord_bytes(f32), G[f"{name}_coord_u8"])
    # the reference drops depth 0 through pts[far] = 1e7 and z < 1e6; no golden pixel is far without being sky
    assert np.array_equal(B.coord_valid_mask_f32(G[f"{name}_depth"], kinv, tf), (G[f"{name}_depth"] != 0).astype(np.uint8))


# ---------------------------------------------------------------------------------------------------
# device buffers with guard bands
# ---------------------------------------------------------------------------------------------------
class Buf:
    def __init__(self, arena, start, dtype, numel, is_output):
        self.arena, self.start, self.dtype, self.numel, self.is_output = arena, start, np.dtype(dtype), numel, is_output
        self.end = start + numel * self.dtype.itemsize
        self.ptr = arena.flat.data_ptr() + start

    def read(self, shape=None):
        a = self.arena.flat[self.start:self.end].cpu().numpy().copy().view(self.dtype)
        return a if shape is None else a.reshape(shape)

    def tensor(self, shape):
        """A contiguous float32 torch view of this buffer (for the Python wrappers)."""
        assert self.dtype == np.float32
        t = self.arena.flat[self.start:self.end].view(torch.float32).view(shape)
        assert t.is_contiguous() and t.data_ptr() == self.ptr
        return t


class Arena:
    """One flat device allocation filled with a sentinel byte; ``carve`` hands out buffers that start ``offset``
    elements past a 256-byte boundary with at least GUARD sentinel bytes on both sides.  ``check`` asserts after a
    launch that every byte outside the output buffers still holds what it held before (sentinel or input data)."""

    def __init__(self, nbytes=1 << 20):
        self.flat = torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device="cuda:0")
        self.cursor, self.bufs = 0, []

    def carve(self, dtype, numel, offset=0, data=None):
        dtype = np.dtype(dtype)
        base = self.flat.data_ptr()
        start = (base + self.cursor + 255) // 256 * 256 - base + GUARD + offset * dtype.itemsize
        buf = Buf(self, start, dtype, int(numel), data is None)
        assert buf.end + GUARD <= self.flat.numel(), "arena too small for this test"
        self.cursor = buf.end + GUARD
        # the residues the kernels' vec predicates look at
        assert buf.ptr % 16 == (offset * dtype.itemsize) % 16 and buf.ptr % 4 == (offset * dtype.itemsize) % 4
        if offset == 1:
            assert buf.ptr % 16 == 4 if dtype.itemsize == 4 else buf.ptr % 4 == dtype.itemsize
        if data is not None:
            src = np.ascontiguousarray(data, dtype=dtype).reshape(-1)
            assert src.size == numel
            self.flat[buf.start:buf.end] = torch.from_numpy(src.view(np.uint8).copy()).to("cuda:0")
        self.bufs.append(buf)
        return buf

    def snapshot(self):
        torch.cuda.synchronize()
        return self.flat.cpu().numpy().copy()

    def check(self, before, written):
        """``written``: the output buffers the launch was given; every other byte must be untouched."""
        after = self.snapshot()
        outside = np.ones(after.size, dtype=bool)
        for b in written:
            assert b.is_output
            outside[b.start:b.end] = False
            for lo, hi, side in ((b.start - GUARD, b.start, "below"), (b.end, b.end + GUARD, "above")):
                bad = np.flatnonzero(after[lo:hi] != SENTINEL)
                assert bad.size == 0, f"guard band {side} a {b.dtype} output overwritten at byte offsets {bad[:8] + lo - b.start}"
        bad = np.flatnonzero((after != before) & outside)
        assert bad.size == 0, f"bytes outside the outputs changed (arena offsets {bad[:8]})"


def _cf(a):
    a = np.asarray(a, dtype=np.float32).reshape(-1)
    return (ctypes.c_float * a.size)(*[float(x) for x in a])


def _lib():
    from infinicube_amd import native
    return native, native.lib(), torch.cuda.current_stream().cuda_stream


def run_coord(depth, kinv, tf, mins, ranges, hv, mis=(), f32=True, u8=True):
    """icv_coord_normalize and icv_coord_valid_mask through the C ABI on guarded buffers; ``mis`` names the pointers
    that start one element off alignment ("depth", "out_f32", "out_u8", "mask").  -> (f32 | None, u8 | None, mask)."""
    native, lib, st = _lib()
    depth = np.ascontiguousarray(depth, dtype=np.float32)
    n, h, w = depth.shape
    ar = Arena()
    off = lambda k: 1 if k in mis else 0   # noqa: E731
    d = ar.carve(np.float32, depth.size, off("depth"), depth)
    t = ar.carve(np.float32, n * 16, 0, np.asarray(tf, dtype=np.float32)[:n])
    of = ar.carve(np.float32, depth.size * 3, off("out_f32")) if f32 else None
    ou = ar.carve(np.uint8, depth.size * 3, off("out_u8")) if u8 else None
    mk = ar.carve(np.uint8, depth.size, off("mask"))
    ck = _cf(kinv)
    before = ar.snapshot()
    native.check(lib.icv_coord_normalize(d.ptr, ck, t.ptr, n, h, w, None if mins is None else _cf(mins),
                                         None if ranges is None else _cf(ranges), hv, of.ptr if f32 else None,
                                         ou.ptr if u8 else None, st), "icv_coord_normalize")
    native.check(lib.icv_coord_valid_mask(d.ptr, ck, t.ptr, n, h, w, mk.ptr, st), "icv_coord_valid_mask")
    ar.check(before, [b for b in (of, ou, mk) if b is not None])
    return (of.read((n, h, w, 3)) if f32 else None, ou.read((n, h, w, 3)) if u8 else None, mk.read((n, h, w)))


def _assert_coord(got, want_f32, want_u8, want_mask):
    f32, u8, mask = got
    if f32 is not None:
        assert np.array_equal(f32, want_f32), f"float32 buffer: {int((f32 != want_f32).sum())} values differ"
    if u8 is not None:
        assert np.array_equal(u8, want_u8), f"uint8 buffer: {int((u8 != want_u8).sum())} bytes differ"
    assert np.array_equal(mask, want_mask), f"valid mask: {int((mask != want_mask).sum())} pixels differ"


RAGGED = [("small", 3, 48, 61), ("small", 3, 48, 62), ("small", 3, 48, 63), ("big", 2, 5, 317)]


def _crop(name, n, h, w):
    return G[f"{name}_depth"][:n, :h, :w], G[f"{name}_coord"][:n, :h, :w], G[f"{name}_coord_u8"][:n, :h, :w]


@pytest.mark.gpu
@pytest.mark.parametrize("name,n,h,w", RAGGED, ids=[f"{c[0]}-W{c[3]}" for c in RAGGED])
def test_coord_ragged_crops_match_reference_golden(name, n, h, w):
    """Cropping the reference fixture on the right (and bottom / back) changes no pixel's (x, y, n), so the expected
    outputs are crops of the reference's own arrays: tails of 1, 2 and 3 pixels (W = 61, 62, 63) and W = 317."""
    depth, want, want_u8 = _crop(name, n, h, w)
    kinv, tf, mins, ranges, hv = _host(name)
    _assert_coord(run_coord(depth, kinv, tf, mins, ranges, hv), want, want_u8, B.coord_valid_mask_f32(depth, kinv, tf[:n]))


@pytest.mark.gpu
@pytest.mark.parametrize("mis", [("depth",), ("out_f32",), ("out_u8",), ("mask",), ("depth", "out_f32", "out_u8", "mask")],
                         ids=["depth", "out_f32", "out_u8", "mask", "all"])
def test_coord_each_misaligned_pointer_takes_the_scalar_path(mis):
    """W = 64: only the pointer alignment can send a thread down the scalar path; each term of ``vec`` on its own."""
    kinv, tf, mins, ranges, hv = _host("small")
    depth = G["small_depth"]
    _assert_coord(run_coord(depth, kinv, tf, mins, ranges, hv, mis=mis), G["small_coord"], G["small_coord_u8"],
                  B.coord_valid_mask_f32(depth, kinv, tf))


@pytest.mark.gpu
@pytest.mark.parametrize("f32,u8", [(True, False), (False, True), (True, True)], ids=["f32", "u8", "both"])
def test_coord_output_selection(f32, u8):
    kinv, tf, mins, ranges, hv = _host("small")
    for w in (64, 62):
        depth, want, want_u8 = _crop("small", 3, 48, w)
        _assert_coord(run_coord(depth, kinv, tf, mins, ranges, hv, f32=f32, u8=u8), want, want_u8,
                      B.coord_valid_mask_f32(depth, kinv, tf))


WIDE = (1024, 1028, 1029, 2051)


@functools.lru_cache(maxsize=None)
def _wide(w):
    """N = 2, H = 3 rows wider than one block: seeded depth in [1, 60] with ~20 % sky and one far pixel (depth 4e6, so
    z >= 1e6: not sky, but outside the sample).  Expected values: the restatement.  Computed once per width."""
    g = np.random.default_rng(1000 + w)
    depth = g.uniform(1.0, 60.0, (2, 3, w)).astype(np.float32)
    depth[g.random((2, 3, w)) < 0.2] = 0
    depth[0, 0, 0], depth[1, 2, w - 1], depth[1, 1, 0] = 7.5, 33.0, 0.0     # corners are known: finite, finite, sky
    far = (1, 1, w - 2)
    depth[far] = 4e6
    kinv, tf = G["small_kinv"], G["small_to_cam0"][:2]
    pts = B.coord_points_f32(depth, kinv, tf)
    mask = B.coord_valid_mask_f32(depth, kinv, tf)
    assert pts[far][2] >= 1e6 and mask[far] == 0 and 0 < mask.sum() < (depth != 0).sum()
    sample = pts[mask.astype(bool)]
    lo, hi = np.quantile(sample, 0.05, axis=0).astype(np.float32), np.quantile(sample, 0.95, axis=0).astype(np.float32)
    mins, ranges = lo, np.maximum(hi - lo, np.float32(1e-7))
    f32 = B.coord_normalize_f32(depth, kinv, tf, mins, ranges, 1)
    out = dict(depth=depth, kinv=kinv, tf=tf, mins=mins, ranges=ranges, pts=pts, mask=mask, f32=f32, u8=B.coord_bytes(f32),
               half=B.coord_normalize_f32(depth, kinv, tf, None, None, 0))
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("w", WIDE)
def test_coord_wide_rows(w):
    """W > 1024 reaches blockIdx.x = 1 (and 2 at W = 2051), with a full last quad (1028) and tails of 1 and 3."""
    c = _wide(w)
    _assert_coord(run_coord(c["depth"], c["kinv"], c["tf"], c["mins"], c["ranges"], 1), c["f32"], c["u8"], c["mask"])


@pytest.mark.gpu
def test_coord_no_valid_point_halves_nonzero_depth():
    """has_valid == 0 with non-zero depth: the kernel emits pt * 0.5 (sky stays 1.0).  float32 only: the bytes of values
    outside [0, 1] are not pinned (numpy's float -> uint8 cast outside [0, 255] is not portable)."""
    kinv, tf = G["small_kinv"], G["small_to_cam0"]
    depth = G["small_depth"][:, :, :61]
    want = B.coord_normalize_f32(depth, kinv, tf, None, None, 0)
    assert (want[depth != 0] != 1.0).any()
    f32, _, _ = run_coord(depth, kinv, tf, None, None, 0, u8=False)
    assert np.array_equal(f32, want)
    c = _wide(1029)
    f32, _, mask = run_coord(c["depth"], c["kinv"], c["tf"], None, None, 0, u8=False)
    assert np.array_equal(f32, c["half"]) and np.array_equal(mask, c["mask"])


def _gather_cases():
    small = G["small_depth"][:, :, :61]
    yield "small-W61", small, G["small_kinv"], G["small_to_cam0"]
    c = _wide(1029)
    yield "wide-W1029", c["depth"], c["kinv"], c["tf"]


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 255, 257, 1000])
def test_coord_gather_points(count):
    """icv_coord_gather_points (the quantile sample of the default device-sampling path) against the restatement's
    points, bit for bit.  The indices always hold pixel 0, the last pixel of the last frame, both ends of a middle row
    and a sky pixel; with one index per launch (count = 1) each of those five is its own launch."""
    native, lib, st = _lib()
    for label, depth, kinv, tf in _gather_cases():
        n, h, w = depth.shape
        total = n * h * w
        pts = B.coord_points_f32(depth, kinv, tf).reshape(total, 3)
        row = ((n // 2) * h + h // 2) * w
        sky = int(np.flatnonzero(depth.reshape(-1) == 0)[0])
        must = [0, total - 1, row, row + w - 1, sky]
        if count == 1:
            index_sets = [np.array([i], dtype=np.int64) for i in must]
        else:
            g = np.random.default_rng(count)
            index_sets = [g.permutation(np.concatenate([must, g.integers(0, total, count - len(must))]).astype(np.int64))]
        ar = Arena()
        d = ar.carve(np.float32, total, 0, depth)
        t = ar.carve(np.float32, n * 16, 0, tf)
        for idx in index_sets:
            assert idx.size == count
            ix = ar.carve(np.int64, count, 0, idx)
            out = ar.carve(np.float32, count * 3)
            before = ar.snapshot()
            native.check(lib.icv_coord_gather_points(d.ptr, _cf(kinv), t.ptr, n, h, w, ix.ptr, count, out.ptr, st), "icv_coord_gather_points")
            ar.check(before, [out])
            got = out.read((count, 3))
            assert np.array_equal(got, pts[idx]), f"{label}: {int((got != pts[idx]).any(axis=1).sum())} of {count} points differ"


# ---------------------------------------------------------------------------------------------------
# icv_semantic_to_color / icv_instance_overlay_u8
# ---------------------------------------------------------------------------------------------------
PIXELS = (1, 2, 3, 5, 1023, 1025, 4099)       # every residue mod 4, both sides of the 1024-pixel block
N_CLASSES = (23, 64, 65, 200)                 # <= 64: the LDS table; above: the table in global memory


def _semantic_case(n, n_classes):
    g = np.random.default_rng(n * 1000 + n_classes)
    lut = g.random((n_classes, 3), dtype=np.float32)
    sem = g.integers(0, n_classes, n).astype(np.int32)
    odd = [-1, n_classes, n_classes + 7, 2 ** 31 - 1]              # all clamp into [0, n_classes - 1]
    r = PIXELS.index(n) if n in PIXELS else 0
    for k, pos in enumerate((0, n // 3, n // 2, n - 1)):            # later positions win: the last pixel is always planted
        sem[pos] = odd[(k + r) % 4]
    want = lut[np.clip(sem, 0, n_classes - 1)]
    return lut, sem, want, (want * np.float32(255)).astype(np.uint8)


def run_semantic(n, n_classes, mis=(), f32=True, u8=True):
    native, lib, st = _lib()
    lut, sem, want, want_u8 = _semantic_case(n, n_classes)
    ar = Arena()
    off = lambda k: 1 if k in mis else 0   # noqa: E731
    s = ar.carve(np.int32, n, off("sem"), sem)
    lt = ar.carve(np.float32, n_classes * 3, 0, lut)
    of = ar.carve(np.float32, n * 3, off("out_f32")) if f32 else None
    ou = ar.carve(np.uint8, n * 3, off("out_u8")) if u8 else None
    before = ar.snapshot()
    native.check(lib.icv_semantic_to_color(s.ptr, n, lt.ptr, n_classes, of.ptr if f32 else None, ou.ptr if u8 else None, st),
                 "icv_semantic_to_color")
    ar.check(before, [b for b in (of, ou) if b is not None])
    if f32:
        got = of.read((n, 3))
        assert np.array_equal(got, want), f"float32 colours differ at pixels {np.flatnonzero((got != want).any(axis=1))[:8]}"
    if u8:
        got = ou.read((n, 3))
        assert np.array_equal(got, want_u8), f"uint8 colours differ at pixels {np.flatnonzero((got != want_u8).any(axis=1))[:8]}"


@pytest.mark.gpu
@pytest.mark.parametrize("n_classes", N_CLASSES)
@pytest.mark.parametrize("n", PIXELS)
def test_semantic_to_color_tails_tables_and_clamp(n, n_classes):
    run_semantic(n, n_classes)


@pytest.mark.gpu
@pytest.mark.parametrize("f32,u8", [(True, False), (False, True)], ids=["f32", "u8"])
def test_semantic_to_color_output_selection(f32, u8):
    for n, n_classes in ((1025, 23), (4099, 200), (3, 65)):
        run_semantic(n, n_classes, f32=f32, u8=u8)


@pytest.mark.gpu
@pytest.mark.parametrize("mis", ["sem", "out_f32", "out_u8"])
def test_semantic_to_color_misaligned_pointer(mis):
    """n = 1024: every thread has a full quad, so only the pointer's alignment selects the scalar path."""
    run_semantic(1024, 23, mis=(mis,))
    run_semantic(1024, 200, mis=(mis,))


def _overlay_case(n):
    g = np.random.default_rng(7000 + n)
    lut = g.integers(0, 256, (65536, 3)).astype(np.uint8)
    lut[0] = (201, 17, 93)                                           # a kernel that painted id 0 would show
    sem_rgb = g.integers(0, 256, (n, 3)).astype(np.uint8)
    special = [0, 7, 65535, 65536, 65536 + 7, -1]                    # k = 0, 7, 65535, 0, 7, 65535
    inst = g.choice(np.array(special + [1, 300, 2 ** 15 + 1, 70000], dtype=np.int64), n).astype(np.int32)
    r = PIXELS.index(n) if n in PIXELS else 0
    for k, pos in enumerate((0, n // 5, n // 3, n // 2, n - 2, n - 1)):
        inst[max(pos, 0)] = special[(k + r) % 6]
    key = inst & 0xffff
    want = np.where((key > 0)[:, None], lut[key], sem_rgb)
    return lut, sem_rgb, inst, want


def run_overlay(n, mis=()):
    native, lib, st = _lib()
    lut, sem_rgb, inst, want = _overlay_case(n)
    ar = Arena()
    off = lambda k: 1 if k in mis else 0   # noqa: E731
    s = ar.carve(np.uint8, n * 3, off("sem_rgb"), sem_rgb)
    i = ar.carve(np.int32, n, off("inst"), inst)
    lt = ar.carve(np.uint8, 65536 * 3, 0, lut)
    out = ar.carve(np.uint8, n * 3, off("out"))
    before = ar.snapshot()
    native.check(lib.icv_instance_overlay_u8(s.ptr, i.ptr, n, lt.ptr, out.ptr, st), "icv_instance_overlay_u8")
    ar.check(before, [out])
    got = out.read((n, 3))
    assert np.array_equal(got, want), f"overlay differs at pixels {np.flatnonzero((got != want).any(axis=1))[:8]}"


@pytest.mark.gpu
@pytest.mark.parametrize("n", PIXELS)
def test_instance_overlay_tails_and_wide_ids(n):
    """ids >= 65536 and negative ids go through ``id & 0xffff``: 65536 keeps the semantic colour, 65536 + 7 takes the
    colour of 7, -1 the colour of 65535."""
    run_overlay(n)


@pytest.mark.gpu
@pytest.mark.parametrize("mis", ["sem_rgb", "out", "inst"])
def test_instance_overlay_misaligned_pointer(mis):
    run_overlay(1024, mis=(mis,))


# ---------------------------------------------------------------------------------------------------
# icv_depth_to_u16 and its wrapper
# ---------------------------------------------------------------------------------------------------
DEPTH_COUNTS = (1, 2, 3, 4, 5, 7) + tuple(range(1021, 1028))


def _depth_case(n, seed=0):
    """Values in [0, 700] (beyond 655.35 numpy's cast wraps modulo 2^16, as tests/test_wire_formats.py relies on)."""
    g = np.random.default_rng(5000 + n + seed)
    d = g.uniform(0.0, 700.0, n).astype(np.float32)
    for pos, v in ((n // 2, 655.35), (n - 1, 655.36), (n // 3, 0.0)):
        d[pos] = v
    return d, (d * np.float32(100)).astype(np.uint16)


@pytest.mark.gpu
@pytest.mark.parametrize("offs", [(0, 0), (1, 0), (0, 1), (3, 3)], ids=["aligned", "depth+1", "out+1", "both+3"])
def test_depth_to_u16_c_abi(offs):
    native, lib, st = _lib()
    for n in DEPTH_COUNTS:
        d, want = _depth_case(n)
        ar = Arena()
        src = ar.carve(np.float32, n, offs[0], d)
        out = ar.carve(np.uint16, n, offs[1])
        before = ar.snapshot()
        native.check(lib.icv_depth_to_u16(src.ptr, n, 100.0, out.ptr, st), "icv_depth_to_u16")
        ar.check(before, [out])
        got = out.read()
        assert np.array_equal(got, want), f"n = {n}: differs at {np.flatnonzero(got != want)[:8]}"


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [1, 3])
def test_depth_wrapper_accepts_offset_device_view(offset):
    """A contiguous device view that starts ``offset`` elements into its allocation is quantised like any other."""
    from infinicube_amd.utils import wire_formats as wf
    for n in DEPTH_COUNTS:
        d, want = _depth_case(n, seed=offset)
        ar = Arena()
        view = ar.carve(np.float32, n, offset, d).tensor((n,))
        assert view.data_ptr() % 16 == 4 * offset
        got = wf.depth_to_uint16_x100(view)
        assert got.dtype == np.uint16 and np.array_equal(got, want), f"n = {n}"


@pytest.mark.gpu
def test_depth_wrapper_accepts_frame_slice_of_odd_sized_buffer():
    """depth[1:] of a (3, 5, 7) device buffer is contiguous and starts 35 elements (140 bytes) into the allocation."""
    from infinicube_amd.utils import wire_formats as wf
    d, want = _depth_case(105)
    dev = torch.from_numpy(d.reshape(3, 5, 7)).to("cuda:0")
    view = dev[1:]
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    got = wf.depth_to_uint16_x100(view)
    assert got.shape == (2, 5, 7) and np.array_equal(got, want.reshape(3, 5, 7)[1:])
    assert np.array_equal(wf.depth_to_uint16_x100(dev), want.reshape(3, 5, 7))


# ---------------------------------------------------------------------------------------------------
# wrapper level: the whole coordinate-buffer function on ragged crops, aligned and misaligned input
# ---------------------------------------------------------------------------------------------------
class Cam:
    def __init__(self, fx, fy, cx, cy):
        self.k = torch.tensor([[float(fx), 0, float(cx)], [0, float(fy), float(cy)], [0, 0, 1]], dtype=torch.float32)

    def get_intrinsics_matrix(self):
        return self.k


@pytest.mark.gpu
@pytest.mark.parametrize("name,h,w", [("small", 47, 61), ("big", 100, 301)])
def test_coordinate_buffer_function_on_ragged_crops(name, h, w):
    """sampling="device" with fewer than 100000 finite points samples every point, so nothing is random.  An aligned
    tensor and a contiguous device view one element off alignment must give identical results, and both sit within the
    bars tests/test_buffers.py uses against another host's LAPACK: float32 within 4 * 2^-24, bytes within +-1 on fewer
    than 1e-3 of them (the oracle's torch ops and this host's inverse / einsum differ from the kernels' in the last bit)."""
    from infinicube_amd.utils.buffer_utils import generate_coordinate_buffer_from_memory_global_norm as gen
    depth = np.ascontiguousarray(G[f"{name}_depth"][:, :h, :w])
    assert 0 < int((depth != 0).sum()) < 100000
    poses, cam = torch.from_numpy(G[f"{name}_poses"]), Cam(*G[f"{name}_intr"])
    torch.manual_seed(0)
    want = B.coordinate_buffer_global_norm(torch.from_numpy(depth), cam.get_intrinsics_matrix(), poses, 0.05).numpy()
    want_u8 = (want * 255).astype(np.uint8)
    aligned = torch.from_numpy(depth).to("cuda:0")
    shifted = Arena().carve(np.float32, depth.size, 1, depth).tensor(depth.shape)
    assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4 and torch.equal(aligned, shifted)
    res = {}
    for label, d in (("aligned", aligned), ("shifted", shifted)):
        res[label] = (gen(d, cam, poses, percentile=0.05, sampling="device").cpu().numpy(),
                      gen(d, cam, poses, percentile=0.05, sampling="device", return_uint8=True).cpu().numpy())
    assert np.array_equal(res["aligned"][0], res["shifted"][0]) and np.array_equal(res["aligned"][1], res["shifted"][1])
    for label, (f32, u8) in res.items():
        err = float(np.abs(f32 - want).max())
        diff = np.abs(u8.astype(np.int16) - want_u8.astype(np.int16))
        print(f"[{name} {h}x{w} {label}] max |f32 - oracle| = {err / 2.0 ** -24:.2f} * 2^-24, {int((diff > 0).sum())} bytes differ")
        assert f32.dtype == np.float32 and err <= 4 * 2.0 ** -24
        assert diff.max() <= 1 and (diff > 0).mean() < 1e-3
