"""The lane maps of the 16x16x32 attention tile (csrc/attn_common.h: attc::tile16, the comment above `struct Tile16`), restated in
plain Python and checked against each other - the one check of that tile a machine without a GPU can run.

What is modelled, from the ISA's operand maps of v_mfma_f32_16x16x32_bf16 (g = lane >> 4, t = lane & 15):
    A[row = t][k = 8 g + j],  B[k = 8 g + j][col = t],  C[row = 4 g + r][col = t]
and of ds_read_b64_tr_b16 (attn_common.h, lds_read_tr16): lane t of a 16-lane group receives, in element j, element (t & 3) of the
four 16-bit values whose address lane 4 j + (t >> 2) of the group supplied.

A 64-key tile is pushed through the whole data path with these maps - the DMA's lane -> (row, source column) mapping into the
swizzled K and V images, the K row reads, the MFMA, the C -> B register hand-over of P, the transposed V reads, the second MFMA - on
integer data, so that any mismatch between P's key order and V's key order, a wrong swizzle or a wrong chunk shows as a wrong number.
"""
import numpy as np
import pytest

D, KVB, NW, NI = 128, 64, 8, 2
LANES = range(64)


# ---- the maps (one function per line of the kernel's comment) --------------------------------------------------------------------
def q_row(qb, lane):
    return 16 * qb + (lane & 15)


def q_frag_d(ks, lane, j):
    return 32 * ks + 8 * (lane >> 4) + j


def k_frag(kb, ks, lane, j):
    """(key, d) of element j of the K fragment read for key block kb, k-step ks."""
    return 16 * kb + (lane & 15), 32 * ks + 8 * (lane >> 4) + j


def st_elem(kb, qb, lane, r):
    """(query, key) of st[kb][qb][r]; the key is also the tail mask's index (plus key0)."""
    return 16 * qb + (lane & 15), 16 * kb + 4 * (lane >> 4) + r


def p_pack(kk, qb, lane, j):
    """(query, key, source (kb, r)) of pf[qb][j] of the 32-key half kk: the MFMA's k index is 8 g + j."""
    kb, r = 2 * kk + (j >> 2), j & 3
    q, key = st_elem(kb, qb, lane, r)
    return q, key, (kb, r)


def v_frag_key(kk, lane, j):
    return 32 * kk + 16 * (j >> 2) + 4 * (lane >> 4) + (j & 3)


def ot_elem(db, qb, lane, r):
    """(query, d) of ot[db][qb][r]."""
    return 16 * qb + (lane & 15), 16 * db + 4 * (lane >> 4) + r


def ot_elem_32(d0, lane, r):
    """the 32x32x16 form (head of attn_common.h): (query, d) of ot[d0][r]."""
    return lane & 31, d0 * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)


# ---- LDS images: what the DMA writes (attn7.hip: "LDS-DMA lane mapping") and the byte offsets the tile reads ----------------------
def dma_image(src, vswz):
    """src [64, 128] -> the tile's LDS image as 64 rows x 16 chunks x 8 elements.  DMA instruction j of wave w: lane -> row
    (w NI + j) 4 + lane / 16, LDS chunk lane & 15 (the hardware adds lane * 16 bytes to a wave-uniform base), source column kcol / vcol."""
    img = np.zeros((KVB * 16 * 8,), dtype=src.dtype)
    for w in range(NW):
        for j in range(NI):
            base = (w * NI + j) * 1024
            for lane in LANES:
                key, pc = (w * NI + j) * 4 + (lane >> 4), lane & 15
                col = (pc ^ ((key & 7) << 1)) * 8 if vswz else (pc ^ (key & 15)) * 8
                o = (base + lane * 16) // 2
                img[o:o + 8] = src[key, col:col + 8]
    return img


def k_read_byte(kb, ks, lane):
    g, t = lane >> 4, lane & 15
    return kb * 4096 + t * 256 + (((ks * 4 + g) ^ t) << 4)


def v_read_byte(kk, jh, db, lane):
    g, t = lane >> 4, lane & 15
    v_row_off = (4 * g + (t >> 2)) * 256
    v_sw = (4 * (g & 1) + (t >> 2)) << 5
    return kk * 8192 + jh * 4096 + v_row_off + ((db * 32 + (t & 3) * 8) ^ v_sw)


def tr_read(img, byte_of_lane):
    """ds_read_b64_tr_b16 of a whole wave: [64 lanes, 4 elements]."""
    out = np.zeros((64, 4), dtype=img.dtype)
    for lane in LANES:
        grp, t = lane & ~15, lane & 15
        for j in range(4):
            src_lane = grp + 4 * j + (t >> 2)
            assert byte_of_lane[src_lane] % 8 == 0
            out[lane, j] = img[byte_of_lane[src_lane] // 2 + (t & 3)]
    return out


def mfma16(a, b, c):
    """a, b [64, 8], c [64, 4] lane registers -> c + A B with the operand maps at the head of this file."""
    A = np.zeros((16, 32), dtype=np.int64)
    B = np.zeros((32, 16), dtype=np.int64)
    for lane in LANES:
        g, t = lane >> 4, lane & 15
        A[t, 8 * g:8 * g + 8] = a[lane]
        B[8 * g:8 * g + 8, t] = b[lane]
    C = A @ B
    out = c.copy()
    for lane in LANES:
        g, t = lane >> 4, lane & 15
        out[lane] += C[4 * g:4 * g + 4, t]
    return out


@pytest.fixture(scope="module")
def tile():
    rng = np.random.default_rng(5)
    return dict(q=rng.integers(-3, 4, (32, D)), k=rng.integers(-3, 4, (KVB, D)), v=rng.integers(-3, 4, (KVB, D)))


def test_every_query_key_pair_of_the_tile_is_produced_once():
    seen = np.zeros((32, KVB), dtype=int)
    for kb in range(4):
        for qb in range(2):
            for lane in LANES:
                for r in range(4):
                    q, key = st_elem(kb, qb, lane, r)
                    seen[q, key] += 1
    assert (seen == 1).all()
    seen_o = np.zeros((32, D), dtype=int)
    for db in range(8):
        for qb in range(2):
            for lane in LANES:
                for r in range(4):
                    q, d = ot_elem(db, qb, lane, r)
                    seen_o[q, d] += 1
    assert (seen_o == 1).all()


def test_p_key_order_equals_v_key_order_for_all_lanes_and_k_steps():
    for kk in range(2):
        covered = np.zeros((2, 32), dtype=int)
        for lane in LANES:
            for j in range(8):
                for qb in range(2):
                    q, key, _ = p_pack(kk, qb, lane, j)
                    assert q == q_row(qb, lane)
                    assert key == v_frag_key(kk, lane, j), (kk, lane, j)
                    assert 32 * kk <= key < 32 * kk + 32
                    if (lane & 15) == 0:
                        covered[qb, key - 32 * kk] += 1
        assert (covered == 1).all(), "a k-step's 32 MFMA k indices must be its 32 keys, each once"


def test_k_image_row_read_returns_the_k_fragment(tile):
    img = dma_image(tile["k"], vswz=False)
    for kb in range(4):
        for ks in range(4):
            for lane in LANES:
                b = k_read_byte(kb, ks, lane)
                assert b % 16 == 0 and 0 <= b <= KVB * 256 - 16
                got = img[b // 2:b // 2 + 8]
                for j in range(8):
                    key, d = k_frag(kb, ks, lane, j)
                    assert got[j] == tile["k"][key, d]


def test_v_image_transposed_read_returns_the_v_fragment(tile):
    img = dma_image(tile["v"], vswz=True)
    for kk in range(2):
        for db in range(8):
            for jh in range(2):
                byte = [v_read_byte(kk, jh, db, lane) for lane in LANES]
                assert all(0 <= b <= KVB * 256 - 8 for b in byte)
                got = tr_read(img, byte)
                for lane in LANES:
                    for jl in range(4):
                        key = v_frag_key(kk, lane, 4 * jh + jl)
                        assert got[lane, jl] == tile["v"][key, 16 * db + (lane & 15)], (kk, db, jh, lane, jl)


def test_the_whole_tile_through_the_maps_equals_the_matrix_products(tile):
    q, k, v = tile["q"], tile["k"], tile["v"]
    kimg, vimg = dma_image(k, False), dma_image(v, True)
    qf = {(qb, ks): np.array([[q[q_row(qb, lane), q_frag_d(ks, lane, j)] for j in range(8)] for lane in LANES]) for qb in range(2) for ks in range(4)}
    st = {}
    for kb in range(4):
        for qb in range(2):
            c = np.zeros((64, 4), dtype=np.int64)
            for ks in range(4):
                kf = np.array([kimg[k_read_byte(kb, ks, lane) // 2:k_read_byte(kb, ks, lane) // 2 + 8] for lane in LANES])
                c = mfma16(kf, qf[(qb, ks)], c)
            st[(kb, qb)] = c
    s_ref = q @ k.T
    for (kb, qb), c in st.items():
        for lane in LANES:
            for r in range(4):
                qq, key = st_elem(kb, qb, lane, r)
                assert c[lane, r] == s_ref[qq, key]
    # "P" = the scores themselves (integers): O^T += V^T P^T
    ot = {(db, qb): np.zeros((64, 4), dtype=np.int64) for db in range(8) for qb in range(2)}
    for kk in range(2):
        pf = {qb: np.array([[st[(2 * kk + (j >> 2), qb)][lane, j & 3] for j in range(8)] for lane in LANES]) for qb in range(2)}
        for db in range(8):
            va = tr_read(vimg, [v_read_byte(kk, 0, db, lane) for lane in LANES])
            vb = tr_read(vimg, [v_read_byte(kk, 1, db, lane) for lane in LANES])
            vf = np.concatenate([va, vb], 1)
            for qb in range(2):
                ot[(db, qb)] = mfma16(vf, pf[qb], ot[(db, qb)])
    o_ref = s_ref @ v
    for (db, qb), c in ot.items():
        for lane in LANES:
            for r in range(4):
                qq, d = ot_elem(db, qb, lane, r)
                assert c[lane, r] == o_ref[qq, d]


@pytest.mark.parametrize("skv", [1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 130])
def test_tail_mask_key_index(skv):
    """key0 + 16 kb + 4 g + r >= skv is masked: exactly the (query, key) pairs whose key lies past the end."""
    nt = (skv + KVB - 1) // KVB
    key0 = (nt - 1) * KVB
    masked = np.zeros((32, KVB), dtype=bool)
    for kb in range(4):
        for qb in range(2):
            for lane in LANES:
                for r in range(4):
                    key_index = key0 + 16 * kb + 4 * (lane >> 4) + r          # the kernel's expression
                    qq, key = st_elem(kb, qb, lane, r)
                    assert key_index == key0 + key
                    masked[qq, key] = key_index >= skv
    want = np.broadcast_to(key0 + np.arange(KVB) >= skv, (32, KVB))
    assert (masked == want).all()


def test_state_overloads_address_the_same_acc_and_ml_elements_as_the_32_form():
    """acc is f32 [Sq, heads * 128], ml [Sq, heads, 2]: either form stores O[q][d] at row q, column head * 128 + d, and the row's
    (m, l) once, from the lanes that hold the first partial of l."""
    heads, head, ldacc, q0 = 3, 2, 3 * 128 + 8, 96

    def addr(row, d):
        return row * ldacc + head * D + d

    a32, a16 = {}, {}
    for lane in LANES:
        hi, l31 = lane >> 5, lane & 31
        base = (q0 + l31) * ldacc + head * D + 4 * hi                      # load_state / store_result, 32 form
        for d0 in range(4):
            for rr in range(4):
                for i in range(4):
                    a = base + d0 * 32 + rr * 8 + i
                    qq, d = ot_elem_32(d0, lane, rr * 4 + i)
                    assert a == addr(q0 + qq, d) and a not in a32
                    a32[a] = (qq, d)
        g, t = lane >> 4, lane & 15
        for qb in range(2):
            base = (q0 + 16 * qb + t) * ldacc + head * D + 4 * g            # the MF = 16 overloads
            for db in range(8):
                for r in range(4):
                    a = base + db * 16 + r
                    qq, d = ot_elem(db, qb, lane, r)
                    assert a == addr(q0 + qq, d) and a not in a16
                    a16[a] = (qq, d)
    assert a32 == a16 and len(a16) == 32 * D
    ml32 = sorted(((q0 + (lane & 31)) * heads + head) * 2 for lane in LANES if lane >> 5 == 0)
    ml16 = sorted(((q0 + 16 * qb + (lane & 15)) * heads + head) * 2 for lane in LANES if lane >> 4 == 0 for qb in range(2))
    assert ml32 == ml16 and len(set(ml16)) == 32


def test_lds_reads_are_bank_conflict_free():
    """Banks are (byte / 4) % 64 for both reads.  ds_read_b128 conflicts inside four 16-lane groups (not contiguous), the transposed
    read inside the two 32-lane halves; identical addresses would broadcast, but none are."""
    g128 = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)), list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))]
    g128 += [[l + 32 for l in g128[0]], [l + 32 for l in g128[1]]]
    for kb in range(4):
        for ks in range(4):
            for grp in g128:
                banks = [(k_read_byte(kb, ks, lane) // 4 + i) % 64 for lane in grp for i in range(4)]
                assert len(set(banks)) == 64
    for kk in range(2):
        for jh in range(2):
            for db in range(8):
                for half in (range(0, 32), range(32, 64)):
                    banks = [(v_read_byte(kk, jh, db, lane) // 4 + i) % 64 for lane in half for i in range(2)]
                    assert len(set(banks)) == 64
