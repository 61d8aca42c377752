"""Operator layer of the DiT host code: thin, checked wrappers that hand torch tensors' device
pointers to the C ABI (include/icvideo.h).  PyTorch is plumbing here (HBM allocation, streams);
every arithmetic op of the denoising loop runs in libicvideo's HIP kernels.

The host driver (dit.py) is written against this small interface so that its sharding / caching
logic can be exercised on CPU by the tests, which inject their own checker implementation
(tests/oracle_ops.py).  The product never does that: ``HipOps`` is the only implementation in this
package and it raises if the native library or a GPU is missing.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import os

import ctypes

import torch

from .. import native
from ..native import EPI_BF16, EPI_F32, EPI_GELU_BF16, EPI_RESID_F32  # noqa: F401 (re-export)

BF16, F32 = torch.bfloat16, torch.float32
FP8 = torch.float8_e4m3fn   # OCP e4m3 (gfx950's fp8), one f32 scale per row next to it


@dataclass
class RopeTable:
    """Per-axis (cos, sin) f32 tables, concatenated [T][22] ++ [Hp][21] ++ [Wp][21] pairs
    (SURVEY.md Appendix A.3); angles are computed in fp64 on the host."""
    table: torch.Tensor  # f32 [(T*22 + Hp*21 + Wp*21), 2]
    T: int
    Hp: int
    Wp: int

    @staticmethod
    def build(T: int, Hp: int, Wp: int, device, head_dim: int = 128, theta: float = 10000.0) -> "RopeTable":
        hw = head_dim // 3
        dims = (head_dim - 2 * hw, hw, hw)
        parts = []
        for axis_dim, n in zip(dims, (T, Hp, Wp)):
            inv = 1.0 / (theta ** (torch.arange(0, axis_dim, 2, dtype=torch.float64)[: axis_dim // 2] / axis_dim))
            ang = torch.outer(torch.arange(n, dtype=torch.float64), inv)
            parts.append(torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1).reshape(-1, 2))
        tab = torch.cat(parts, dim=0).to(torch.float32).contiguous().to(device)
        return RopeTable(tab, T, Hp, Wp)


def _chk(t: torch.Tensor, dtype, name: str, last_contig: bool = True):
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if last_contig and t.dim() >= 1 and t.stride(-1) != 1:
        raise ValueError(f"{name}: innermost dimension must be contiguous")


class HipOps:
    """The product operator set: every method enqueues one libicvideo kernel on the current
    HIP stream of ``device``."""

    name = "hip"

    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise native.NativeError(
                f"HipOps needs a ROCm GPU device ('cuda:N'), got {device!r}; there is no CPU fallback")
        if not torch.cuda.is_available():
            raise native.NativeError("HipOps: no GPU visible to PyTorch-ROCm; there is no CPU fallback")
        self.lib = native.lib()
        # one process drives one GPU: kernels are launched on this device's current stream and the library keeps
        # per-process (not per-device) launch attributes, so make it the process's current HIP device
        torch.cuda.set_device(self.device)
        # kernel A/B switches (icv_set_option) from the environment, e.g. ICV_OPTIONS="attn2_variant=4,gemm256=1"
        for item in filter(None, os.environ.get("ICV_OPTIONS", "").split(",")):
            name, _, val = item.partition("=")
            native.check(self.lib.icv_set_option(name.strip().encode(), int(val)), f"icv_set_option({item})")

    # -- helpers ---------------------------------------------------------------------------
    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def alloc(self, shape, dtype) -> torch.Tensor:
        return torch.empty(shape, dtype=dtype, device=self.device)

    def to_device(self, t: torch.Tensor, dtype) -> torch.Tensor:
        return t.detach().to(device=self.device, dtype=dtype).contiguous()

    # -- kernels ---------------------------------------------------------------------------
    def gemm(self, a, w, bias, out, epilogue, resid=None, gate=None, nsplit=None):
        """out = epilogue(a @ w.T + bias).  a [M,K] bf16, w [N,K] bf16, bias f32[N] | None.
        ``out`` is [M,N] (bf16 or f32 by epilogue), or [N/nsplit, M, nsplit] when nsplit is set."""
        _chk(a, BF16, "gemm.a"); _chk(w, BF16, "gemm.w")
        M, K = a.shape
        N = w.shape[0]
        if w.shape[1] != K:
            raise ValueError(f"gemm: K mismatch {a.shape} x {w.shape}")
        want = BF16 if epilogue in (EPI_BF16, EPI_GELU_BF16) else F32
        _chk(out, want, "gemm.out")
        if nsplit is None:
            if tuple(out.shape) != (M, N):
                raise ValueError(f"gemm: out shape {tuple(out.shape)} != {(M, N)}")
            ldo, ns, sstride = out.stride(0), N, 0
        else:
            if tuple(out.shape) != (N // nsplit, M, nsplit):
                raise ValueError(f"gemm: split out shape {tuple(out.shape)} != {(N // nsplit, M, nsplit)}")
            ldo, ns, sstride = out.stride(1), nsplit, out.stride(0)
        if bias is not None:
            _chk(bias, F32, "gemm.bias")
        if resid is not None:
            _chk(resid, F32, "gemm.resid")
        if gate is not None:
            _chk(gate, F32, "gemm.gate")
        native.check(self.lib.icv_gemm_bf16(
            a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), native.ptr(bias), M, N, K, epilogue,
            out.data_ptr(), ldo, ns, sstride, native.ptr(resid),
            resid.stride(0) if resid is not None else 0, native.ptr(gate), self._stream()), "icv_gemm_bf16")

    def gemv(self, x, w, bias, out, in_act=0, out_act=0):
        _chk(x, F32, "gemv.x"); _chk(w, BF16, "gemv.w"); _chk(out, F32, "gemv.out")
        M, K = x.shape
        N = w.shape[0]
        assert x.is_contiguous() and w.is_contiguous() and out.is_contiguous() and tuple(out.shape) == (M, N)
        native.check(self.lib.icv_gemv_f32(x.data_ptr(), w.data_ptr(), native.ptr(bias), out.data_ptr(),
                                           M, N, K, in_act, out_act, self._stream()), "icv_gemv_f32")

    def sinusoidal(self, timestep: float, out):
        _chk(out, F32, "sinusoidal.out")
        native.check(self.lib.icv_sinusoidal_embedding(float(timestep), out.numel(), out.data_ptr(),
                                                       self._stream()), "icv_sinusoidal_embedding")

    def bcast_add(self, a, b, out):
        _chk(a, F32, "bcast_add.a"); _chk(b, F32, "bcast_add.b"); _chk(out, F32, "bcast_add.out")
        assert a.is_contiguous() and b.is_contiguous() and out.is_contiguous()
        rows, n = a.numel() // b.numel(), b.numel()
        native.check(self.lib.icv_bcast_add_f32(a.data_ptr(), b.data_ptr(), out.data_ptr(), rows, n,
                                                self._stream()), "icv_bcast_add_f32")

    def ln_modulate(self, x, out, weight=None, bias=None, shift=None, scale=None, eps=1e-6):
        _chk(x, F32, "ln.x"); _chk(out, BF16, "ln.out")
        rows, d = x.shape
        native.check(self.lib.icv_ln_modulate(
            x.data_ptr(), x.stride(0), native.ptr(weight), native.ptr(bias), native.ptr(shift),
            native.ptr(scale), out.data_ptr(), out.stride(0), rows, d, eps, self._stream()), "icv_ln_modulate")

    # ---- fp8 path (BASELINE.json config #5): e4m3 rows + one f32 scale per row ----------------------
    def quantize_rows(self, src, out_q, out_scale):
        """src bf16|f32 [rows, K] -> out_q e4m3 [rows, K], out_scale f32 [rows] (row abs-max / 448)."""
        if src.dtype not in (BF16, F32):
            raise TypeError(f"quantize_rows.src: expected bf16 or f32, got {src.dtype}")
        _chk(src, src.dtype, "quantize_rows.src"); _chk(out_q, FP8, "quantize_rows.out"); _chk(out_scale, F32, "quantize_rows.scale")
        rows, K = src.shape
        assert tuple(out_q.shape) == (rows, K) and out_scale.numel() == rows and out_scale.is_contiguous()
        native.check(self.lib.icv_quantize_rows_fp8(
            src.data_ptr(), int(src.dtype == F32), src.stride(0), rows, K, out_q.data_ptr(), out_q.stride(0),
            out_scale.data_ptr(), self._stream()), "icv_quantize_rows_fp8")

    def ln_modulate_fp8(self, x, out_q, out_scale, weight=None, bias=None, shift=None, scale=None, eps=1e-6):
        _chk(x, F32, "ln8.x"); _chk(out_q, FP8, "ln8.out"); _chk(out_scale, F32, "ln8.scale")
        rows, d = x.shape
        assert tuple(out_q.shape) == (rows, d) and out_scale.numel() == rows and out_scale.is_contiguous()
        native.check(self.lib.icv_ln_modulate_fp8(
            x.data_ptr(), x.stride(0), native.ptr(weight), native.ptr(bias), native.ptr(shift),
            native.ptr(scale), out_q.data_ptr(), out_q.stride(0), out_scale.data_ptr(), rows, d, eps,
            self._stream()), "icv_ln_modulate_fp8")

    def gemm_fp8(self, a_q, a_scale, w_q, w_scale, bias, out, epilogue, resid=None, gate=None, nsplit=None):
        """out = epilogue((a_q @ w_q.T) * a_scale[:, None] * w_scale[None, :] + bias); shapes as ``gemm``."""
        _chk(a_q, FP8, "gemm8.a"); _chk(w_q, FP8, "gemm8.w"); _chk(a_scale, F32, "gemm8.a_scale"); _chk(w_scale, F32, "gemm8.w_scale")
        M, K = a_q.shape
        N = w_q.shape[0]
        if w_q.shape[1] != K:
            raise ValueError(f"gemm_fp8: K mismatch {a_q.shape} x {w_q.shape}")
        assert a_scale.numel() == M and w_scale.numel() == N and a_scale.is_contiguous() and w_scale.is_contiguous()
        want = BF16 if epilogue in (EPI_BF16, EPI_GELU_BF16) else F32
        _chk(out, want, "gemm8.out")
        if nsplit is None:
            if tuple(out.shape) != (M, N):
                raise ValueError(f"gemm_fp8: out shape {tuple(out.shape)} != {(M, N)}")
            ldo, ns, sstride = out.stride(0), N, 0
        else:
            if tuple(out.shape) != (N // nsplit, M, nsplit):
                raise ValueError(f"gemm_fp8: split out shape {tuple(out.shape)} != {(N // nsplit, M, nsplit)}")
            ldo, ns, sstride = out.stride(1), nsplit, out.stride(0)
        for t, nm in ((bias, "bias"), (resid, "resid"), (gate, "gate")):
            if t is not None:
                _chk(t, F32, f"gemm8.{nm}")
        native.check(self.lib.icv_gemm_fp8(
            a_q.data_ptr(), a_q.stride(0), a_scale.data_ptr(), w_q.data_ptr(), w_q.stride(0), w_scale.data_ptr(),
            native.ptr(bias), M, N, K, epilogue, out.data_ptr(), ldo, ns, sstride, native.ptr(resid),
            resid.stride(0) if resid is not None else 0, native.ptr(gate), self._stream()), "icv_gemm_fp8")

    def rmsnorm_rope(self, x0, w0, x1=None, w1=None, eps=1e-6, rope: Optional[RopeTable] = None, tok0=0):
        _chk(x0, BF16, "rms.x0"); _chk(w0, F32, "rms.w0")
        rows, d = x0.shape
        ld = x0.stride(0)
        if x1 is not None:
            _chk(x1, BF16, "rms.x1"); _chk(w1, F32, "rms.w1")
            assert x1.shape == x0.shape and x1.stride(0) == ld
        native.check(self.lib.icv_rmsnorm_rope(
            x0.data_ptr(), w0.data_ptr(), native.ptr(x1), native.ptr(w1), ld, rows, d, eps,
            rope.table.data_ptr() if rope is not None else None,
            rope.T if rope else 0, rope.Hp if rope else 0, rope.Wp if rope else 0, tok0,
            self._stream()), "icv_rmsnorm_rope")

    def attention(self, q, k, v, o, heads: int, scale: float):
        for t, nm in ((q, "q"), (k, "k"), (v, "v"), (o, "o")):
            _chk(t, BF16, f"attention.{nm}")
        native.check(self.lib.icv_attention_fwd(
            q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0),
            o.data_ptr(), o.stride(0), q.shape[0], k.shape[0], heads, scale, self._stream()),
            "icv_attention_fwd")

    def attention_add(self, q, k, v, o, heads: int, scale: float):
        """o += softmax(q k^T * scale) v  (i2v image cross-attention summed onto the text one)."""
        for t, nm in ((q, "q"), (k, "k"), (v, "v"), (o, "o")):
            _chk(t, BF16, f"attention_add.{nm}")
        native.check(self.lib.icv_attention_fwd_add(
            q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0),
            o.data_ptr(), o.stride(0), q.shape[0], k.shape[0], heads, scale, self._stream()),
            "icv_attention_fwd_add")

    # ---- fp8 attention (fp8 mode only): e4m3 Q/K/V/P on the K=64 scaled MFMA ----------------------------------
    def attention_fp8_buffers(self, Sq: int, Skv: int, d: int, heads: int):
        """Workspace of attention_fp8: (qq [Sq,d], kq [Skv,d], vt bytes, amax f32 [3, heads])."""
        nbytes = int(self.lib.icv_attention_fp8_vt_bytes(Skv, heads))
        return (self.alloc((Sq, d), FP8), self.alloc((Skv, d), FP8), self.alloc((nbytes,), torch.uint8), self.alloc((3, heads), F32))

    def attention_fp8_prepare(self, ws, heads: int, q=None, k=None, v=None):
        """Quantise the queries and / or the keys + values of one attention into the workspace (per-head power-of-two
        scales from the abs-max, e4m3 rows, transposed key-permuted V tiles)."""
        qq, kq, vt, amax = ws
        if q is not None:
            _chk(q, BF16, "attention_fp8.q"); assert qq.shape[0] >= q.shape[0] and qq.shape[1] == q.shape[1]
        if k is not None:
            _chk(k, BF16, "attention_fp8.k"); _chk(v, BF16, "attention_fp8.v")
            assert kq.shape[0] >= k.shape[0] and kq.shape[1] == k.shape[1] and v.shape == k.shape
            assert vt.numel() >= int(self.lib.icv_attention_fp8_vt_bytes(k.shape[0], heads))
        native.check(self.lib.icv_attention_fp8_prepare(
            native.ptr(q), q.stride(0) if q is not None else 0, native.ptr(k), k.stride(0) if k is not None else 0,
            native.ptr(v), v.stride(0) if v is not None else 0, q.shape[0] if q is not None else 0,
            k.shape[0] if k is not None else 0, heads, qq.data_ptr() if q is not None else None, qq.stride(0),
            kq.data_ptr() if k is not None else None, kq.stride(0), vt.data_ptr() if k is not None else None,
            amax.data_ptr(), self._stream()), "icv_attention_fp8_prepare")

    def attention_fp8(self, q, k, v, o, heads: int, ws):
        """o = softmax2(q k^T) v with e4m3 operands; K must carry scale * log2(e) (the DiT's unit-scale convention).
        ``ws`` = attention_fp8_buffers(...) sized for these shapes."""
        _chk(o, BF16, "attention_fp8.o")
        self.attention_fp8_prepare(ws, heads, q=q, k=k, v=v)
        qq, kq, vt, amax = ws
        native.check(self.lib.icv_attention_fp8_fwd(
            qq.data_ptr(), qq.stride(0), kq.data_ptr(), kq.stride(0), vt.data_ptr(), amax.data_ptr(), o.data_ptr(), o.stride(0),
            q.shape[0], k.shape[0], heads, self._stream()), "icv_attention_fp8_fwd")

    def attention_fp8_chunk(self, ws, Sq: int, Skv: int, o, acc, ml, heads: int, first: bool, last: bool):
        """fp8 attention of the prepared queries over the prepared chunk of keys / values, carried state as
        attention_chunk (acc f32 [Sq, H*128], ml f32 [Sq, H, 2])."""
        qq, kq, vt, amax = ws
        if o is not None:
            _chk(o, BF16, "attention_fp8_chunk.o")
        native.check(self.lib.icv_attention_fp8_fwd_chunk(
            qq.data_ptr(), qq.stride(0), kq.data_ptr(), kq.stride(0), vt.data_ptr(), amax.data_ptr(), native.ptr(o),
            o.stride(0) if o is not None else 0, native.ptr(acc), acc.stride(0) if acc is not None else 0, native.ptr(ml),
            Sq, Skv, heads, int(first), int(last), self._stream()), "icv_attention_fp8_fwd_chunk")

    # e4m3 K|V on the wire (sequence parallel): quantise the LOCAL rows once, exchange e4m3 blobs, attend over the pieces
    def attention_fp8_blob_bytes(self, rows: int, heads: int) -> int:
        return int(self.lib.icv_attention_fp8_blob_bytes(rows, heads))

    def attention_fp8_kv_amax(self, k, v, heads: int, amax):
        """amax f32 [3, H]: rows 1 / 2 <- per-head abs-max of this rank's k / v rows (row 0, the queries', is left alone)."""
        _chk(k, BF16, "attention_fp8_kv_amax.k"); _chk(v, BF16, "attention_fp8_kv_amax.v"); _chk(amax, F32, "attention_fp8_kv_amax.amax")
        native.check(self.lib.icv_attention_fp8_kv_amax(k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), k.shape[0], heads, amax.data_ptr(),
                                                        self._stream()), "icv_attention_fp8_kv_amax")

    def attention_fp8_quantize_kv(self, k, v, heads: int, amax, blob):
        """rows of k / v -> one e4m3 blob (kq rows | transposed V tiles) with the per-head scales of ``amax``."""
        assert blob.dtype == torch.uint8 and blob.is_contiguous() and blob.numel() >= self.attention_fp8_blob_bytes(k.shape[0], heads)
        native.check(self.lib.icv_attention_fp8_quantize_kv(k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), k.shape[0], heads, amax.data_ptr(),
                                                            blob.data_ptr(), self._stream()), "icv_attention_fp8_quantize_kv")

    def attention_fp8_pieces(self, ws, amax, blobs, piece_rows: int, n_pieces: int, Sq: int, o, acc, ml, heads: int, first: bool, last: bool, gate=None):
        """fp8 attention of the prepared queries (ws) over ``n_pieces`` blobs back to back (the gathered chunk), carried state as
        attention_chunk.  ``gate`` (arrival-driven, icv_attention_fp8_fwd_pieces_gated): dict(seq=[(piece, flag, value), ...] - the order in
        which the pieces are walked, this rank's own first; flag < 0 = there now, else readable once (int32)(flags[flag] - value) >= 0 -,
        flags=device words, own=(uint8 tensor, index) or None: that piece is read from the tensor instead of its slot in ``blobs``,
        err=int32 device word or None, timeout_us)."""
        qq = ws[0]
        assert blobs.dtype == torch.uint8 and blobs.is_contiguous() and blobs.numel() >= n_pieces * self.attention_fp8_blob_bytes(piece_rows, heads)
        if gate is not None:
            seq = gate["seq"]
            assert len(seq) == n_pieces
            sp = (ctypes.c_int32 * n_pieces)(*[int(e[0]) for e in seq])
            sf = (ctypes.c_int32 * n_pieces)(*[int(e[1]) for e in seq])
            sv = (ctypes.c_uint32 * n_pieces)(*[int(e[2]) & 0xffffffff for e in seq])
            own = gate.get("own")
            own_t, own_i = own if own is not None else (None, -1)
            if own_t is not None:
                assert own_t.dtype == torch.uint8 and own_t.is_contiguous() and own_t.numel() >= self.attention_fp8_blob_bytes(piece_rows, heads)
            native.check(self.lib.icv_attention_fp8_fwd_pieces_gated(
                qq.data_ptr(), qq.stride(0), blobs.data_ptr(), piece_rows, n_pieces, native.ptr(own_t), int(own_i), ctypes.cast(sp, ctypes.c_void_p),
                ctypes.cast(sf, ctypes.c_void_p), ctypes.cast(sv, ctypes.c_void_p), native.ptr(gate.get("flags")), native.ptr(gate.get("err")),
                int(gate.get("timeout_us", 0)), amax.data_ptr(), native.ptr(o), o.stride(0) if o is not None else 0, native.ptr(acc),
                acc.stride(0) if acc is not None else 0, native.ptr(ml), Sq, heads, int(first), int(last), self._stream()),
                "icv_attention_fp8_fwd_pieces_gated")
            return
        native.check(self.lib.icv_attention_fp8_fwd_pieces(
            qq.data_ptr(), qq.stride(0), blobs.data_ptr(), piece_rows, n_pieces, amax.data_ptr(), native.ptr(o), o.stride(0) if o is not None else 0,
            native.ptr(acc), acc.stride(0) if acc is not None else 0, native.ptr(ml), Sq, heads, int(first), int(last), self._stream()),
            "icv_attention_fp8_fwd_pieces")

    def attention_fp8_with_amax(self, ws, amax):
        """The same workspace with another abs-max table (one per CFG branch: the branches' K / V scales differ)."""
        return (ws[0], ws[1], ws[2], amax)

    def attention_chunk(self, q, k, v, o, acc, ml, heads: int, scale: float, first: bool, last: bool):
        """Attention over one chunk of keys with carried softmax state (acc f32 [Sq, H*128], ml f32
        [Sq, H, 2]); ``first`` starts from the empty state, ``last`` normalises into ``o``."""
        for t, nm in ((q, "q"), (k, "k"), (v, "v")):
            _chk(t, BF16, f"attention_chunk.{nm}")
        if o is not None:
            _chk(o, BF16, "attention_chunk.o")
        if acc is not None:
            _chk(acc, F32, "attention_chunk.acc"); _chk(ml, F32, "attention_chunk.ml")
            assert ml.is_contiguous() and tuple(ml.shape) == (q.shape[0], heads, 2)
        native.check(self.lib.icv_attention_fwd_chunk(
            q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0),
            native.ptr(o), o.stride(0) if o is not None else 0, native.ptr(acc),
            acc.stride(0) if acc is not None else 0, native.ptr(ml), q.shape[0], k.shape[0], heads, scale,
            int(first), int(last), self._stream()), "icv_attention_fwd_chunk")

    def attention_pieces(self, q, pieces, o, heads: int, scale: float, flags=None, err=None, timeout_us: int = 0, trace=None):
        """K6, arrival-driven (csrc/attn7p.hip): ONE launch over the K|V ``pieces`` = [(k, v, flag, value), ...] - k, v bf16 row views
        with one common row stride each; flag < 0: the rows are in place now (this rank's own rows: list them FIRST); otherwise the rows
        are there once (int32)(flags[flag] - value) >= 0 (``flags`` int32 / uint32 device tensor written behind the transfer).  A piece
        that is late costs a bounded in-kernel wait; after ``timeout_us`` the kernel stores 0x80000000 | piece into ``err`` and goes on."""
        _chk(q, BF16, "attention_pieces.q"); _chk(o, BF16, "attention_pieces.o")
        arr = (native.KVPiece * len(pieces))()
        ldk = ldv = None
        for i, (k, v, flag, value) in enumerate(pieces):
            if k.shape[0] == 0:
                arr[i] = native.KVPiece(None, None, 0, -1, 0)
                continue
            _chk(k, BF16, "attention_pieces.k"); _chk(v, BF16, "attention_pieces.v")
            assert ldk in (None, k.stride(0)) and ldv in (None, v.stride(0)), "attention_pieces: the pieces must share their row strides"
            ldk, ldv = k.stride(0), v.stride(0)
            arr[i] = native.KVPiece(k.data_ptr(), v.data_ptr(), k.shape[0], int(flag), int(value) & 0xffffffff)
        native.check(self.lib.icv_attention_fwd_pieces(
            q.data_ptr(), q.stride(0), ctypes.cast(arr, ctypes.c_void_p), len(pieces), ldk or 0, ldv or 0, o.data_ptr(), o.stride(0), q.shape[0], heads, scale,
            native.ptr(flags), native.ptr(err), int(timeout_us), native.ptr(trace), self._stream()), "icv_attention_fwd_pieces")

    def attention_framewin(self, q, k, v, o, heads: int, scale: float, frames: int, frame_rows: int, window: int, sink: int):
        """K6, frame-windowed (csrc/attn7p.hip): ONE launch in which the queries of latent frame f (``frame_rows``
        contiguous rows) read the keys of the frames within ``window`` of f plus the first ``sink`` frames."""
        for t, nm in ((q, "q"), (k, "k"), (v, "v"), (o, "o")):
            _chk(t, BF16, f"attention_framewin.{nm}")
        rows = frames * frame_rows
        if not (q.shape[0] == k.shape[0] == v.shape[0] == rows and o.shape[0] >= rows):
            raise ValueError(f"attention_framewin: {frames} frames of {frame_rows} rows, but q / k / v / o have "
                             f"{q.shape[0]} / {k.shape[0]} / {v.shape[0]} / {o.shape[0]} rows")
        native.check(self.lib.icv_attention_fwd_framewin(
            q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), o.data_ptr(), o.stride(0),
            frames, frame_rows, heads, window, sink, scale, self._stream()), "icv_attention_fwd_framewin")

    def attention_radial(self, q, k, v, o, heads: int, scale: float, frames: int, frame_rows: int, window: int, sink: int):
        """K6, radial (csrc/attn7r.hip; the rule: attn_window.radial_ranges): ONE launch in which a 256-row query block
        of latent frame f reads every key frame - whole within ``window`` of f and for the first ``sink`` frames, else a band of
        in-frame rows around its own that halves with every doubling of the temporal distance."""
        for t, nm in ((q, "q"), (k, "k"), (v, "v"), (o, "o")):
            _chk(t, BF16, f"attention_radial.{nm}")
        rows = frames * frame_rows
        if not (q.shape[0] == k.shape[0] == v.shape[0] == rows and o.shape[0] >= rows):
            raise ValueError(f"attention_radial: {frames} frames of {frame_rows} rows, but q / k / v / o have "
                             f"{q.shape[0]} / {k.shape[0]} / {v.shape[0]} / {o.shape[0]} rows")
        native.check(self.lib.icv_attention_fwd_radial(
            q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), o.data_ptr(), o.stride(0),
            frames, frame_rows, heads, window, sink, scale, self._stream()), "icv_attention_fwd_radial")

    def flag_write(self, flags, index: int, value: int, delay_us: int = 0, stream: Optional[int] = None):
        """flags[index] <- value (system-scope release) on ``stream`` (default: the current one), optionally after holding it delay_us."""
        assert flags.dtype in (torch.int32, torch.uint32) and flags.is_contiguous()
        native.check(self.lib.icv_flag_write(flags.data_ptr(), index, int(value) & 0xffffffff, int(delay_us),
                                             self._stream() if stream is None else stream), "icv_flag_write")

    def patchify(self, latent, out, tok0: int, n_tok: int):
        _chk(latent, F32, "patchify.latent"); _chk(out, BF16, "patchify.out")
        assert latent.is_contiguous()
        C, T, H8, W8 = latent.shape
        native.check(self.lib.icv_patchify(latent.data_ptr(), C, T, H8, W8, out.data_ptr(),
                                           out.stride(0), tok0, n_tok, self._stream()), "icv_patchify")

    def unpatchify_cfg_euler(self, latent, hc, hu, cfg_scale, dsigma, tok0, n_tok, vel_out=None, round_bf16=False):
        _chk(latent, F32, "euler.latent"); _chk(hc, F32, "euler.hc")
        assert latent.is_contiguous()
        C, T, H8, W8 = latent.shape
        native.check(self.lib.icv_unpatchify_cfg_euler(
            latent.data_ptr(), native.ptr(vel_out), hc.data_ptr(), native.ptr(hu), hc.stride(0),
            cfg_scale, dsigma, C, T, H8, W8, tok0, n_tok, int(bool(round_bf16)), self._stream()), "icv_unpatchify_cfg_euler")

    def unpatchify_cfg_multistep(self, latent, x_hat, m_new, m_prev, m_prev2, hc, hu, cfg_scale, sigma, a, c, tok0, n_tok, round_bf16=False):
        """Multistep samplers (solver.py): for the local tokens, m_new = latent - sigma * CFG(hc, hu); x_hat <- x_c = a . (x_hat, m_prev,
        m_prev2, m_new) (``a`` None: x_c = latent); latent <- c . (x_c, m_new, m_prev).  Five different f32 latent-shaped buffers;
        m_prev / m_prev2 may be None where their coefficients are 0."""
        bufs = dict(latent=latent, x_hat=x_hat, m_new=m_new, m_prev=m_prev, m_prev2=m_prev2)
        for name, t in bufs.items():
            if t is None and name in ("m_prev", "m_prev2"):
                continue
            _chk(t, F32, f"multistep.{name}")
            if not t.is_contiguous() or tuple(t.shape) != tuple(latent.shape):
                raise ValueError(f"unpatchify_cfg_multistep: {name} must be a contiguous tensor of the latent's shape {tuple(latent.shape)}")
        _chk(hc, F32, "multistep.hc")
        if hc.shape[0] < n_tok or (hu is not None and (hu.shape[0] < n_tok or hu.stride(0) != hc.stride(0))):
            raise ValueError("unpatchify_cfg_multistep: head outputs have fewer rows than n_tok (or differ in row stride)")
        C, T, H8, W8 = latent.shape
        a4 = (0.0, 0.0, 0.0, 0.0) if a is None else tuple(float(x) for x in a)
        c3 = tuple(float(x) for x in c)
        native.check(self.lib.icv_unpatchify_cfg_multistep(
            latent.data_ptr(), x_hat.data_ptr(), m_new.data_ptr(), native.ptr(m_prev), native.ptr(m_prev2), hc.data_ptr(), native.ptr(hu),
            hc.stride(0), cfg_scale, float(sigma), int(a is not None), *a4, *c3, C, T, H8, W8, tok0, n_tok, int(bool(round_bf16)),
            self._stream()), "icv_unpatchify_cfg_multistep")

    def cfg_zero_scale(self, hc, hu, n_tok, workspace, scale_out, round_bf16=False):
        """CFG-Zero* optimised scale (guidance.py): over the first n_tok rows of the head outputs hc, hu (f32 [>= n_tok, 4*C], equal
        row strides), scale_out[0] = s = <hc, hu> / (|hu|^2 + 1e-8) and hu <- s * hu IN PLACE (icv_cfg_zero_scale_f32: fp64 sums, two
        launches, no host read).  workspace: f64 [ICV_CFG_ZERO_WORKSPACE_DOUBLES]; scale_out: f32, one element."""
        _chk(hc, F32, "cfg_zero_scale.hc"); _chk(hu, F32, "cfg_zero_scale.hu"); _chk(scale_out, F32, "cfg_zero_scale.scale_out")
        _chk(workspace, torch.float64, "cfg_zero_scale.workspace")
        if hc.dim() != 2 or hu.dim() != 2 or hc.shape[1] != hu.shape[1] or hc.shape[0] < n_tok or hu.shape[0] < n_tok or hu.stride(0) != hc.stride(0):
            raise ValueError("cfg_zero_scale: head outputs have fewer rows than n_tok (or differ in width or row stride)")
        if workspace.numel() < native.CFG_ZERO_WORKSPACE_DOUBLES or not workspace.is_contiguous() or scale_out.numel() != 1:
            raise ValueError(f"cfg_zero_scale: workspace must hold {native.CFG_ZERO_WORKSPACE_DOUBLES} contiguous doubles and scale_out one float")
        native.check(self.lib.icv_cfg_zero_scale_f32(hc.data_ptr(), hu.data_ptr(), hc.stride(0), n_tok, hc.shape[1], workspace.data_ptr(),
                                                     scale_out.data_ptr(), int(bool(round_bf16)), self._stream()), "icv_cfg_zero_scale_f32")

    def nag_combine(self, zp, zn, out, scale, tau, alpha):
        """Normalized Attention Guidance (nag.py): zp, zn, out bf16 [rows, d] (row strides allowed); per row, in f32,
        g = scale * zp - (scale - 1) * zn, c = min(|g|_1 / |zp|_1, tau) / (|g|_1 / |zp|_1), out = alpha * c * g + (1 - alpha) * zp
        (icv_nag_combine_bf16: the row stays in registers, so ``out`` may be ``zp`` itself)."""
        _chk(zp, BF16, "nag_combine.zp"); _chk(zn, BF16, "nag_combine.zn"); _chk(out, BF16, "nag_combine.out")
        if zp.dim() != 2 or tuple(zn.shape) != tuple(zp.shape) or tuple(out.shape) != tuple(zp.shape):
            raise ValueError(f"nag_combine: zp, zn and out must be [rows, d] of one shape, got {tuple(zp.shape)}, {tuple(zn.shape)}, {tuple(out.shape)}")
        rows, d = zp.shape
        if rows == 0 or d % 256 or d > 8192 or any(t.stride(0) % 8 or t.data_ptr() % 16 for t in (zp, zn, out)):
            raise ValueError(f"nag_combine: needs rows > 0, d % 256 == 0 and d <= 8192 (got {rows} x {d}), row strides that are multiples "
                             "of 8 and 16-byte-aligned rows")
        native.check(self.lib.icv_nag_combine_bf16(zp.data_ptr(), zp.stride(0), zn.data_ptr(), zn.stride(0), out.data_ptr(), out.stride(0),
                                                   rows, d, float(scale), float(tau), float(alpha), self._stream()), "icv_nag_combine_bf16")

    def enhance_scores(self, q, k, frames: int, frame_rows: int, heads: int, scale: float, weight: float, workspace, score_out=None):
        """Enhance-A-Video (enhance.py): q, k bf16 [frames * frame_rows, heads * 128] (row strides allowed), the operands of
        ``attention``.  Per position and head the frames x frames softmax of scale * <q, k> over the frames of that position; the
        off-diagonal mass of every position goes to ``workspace`` (f32 [>= frame_rows], contiguous) for ``enhance_apply``
        (icv_enhance_scores_bf16).  ``score_out`` (f32, one element): also E = max(1, (frames + weight) * mean)."""
        _chk(q, BF16, "enhance_scores.q"); _chk(k, BF16, "enhance_scores.k"); _chk(workspace, F32, "enhance_scores.workspace")
        rows = frames * frame_rows
        if q.dim() != 2 or tuple(k.shape) != tuple(q.shape) or q.shape[0] != rows or q.shape[1] != heads * 128:
            raise ValueError(f"enhance_scores: q and k must be [{frames} frames * {frame_rows} rows, {heads} heads * 128], got "
                             f"{tuple(q.shape)}, {tuple(k.shape)}")
        if not 2 <= frames <= 32:
            raise ValueError(f"enhance_scores: needs 2 <= frames <= 32, got {frames}")
        if any(t.stride(0) % 8 or t.data_ptr() % 16 for t in (q, k)):
            raise ValueError("enhance_scores: needs row strides that are multiples of 8 and 16-byte-aligned rows")
        self._enhance_buffers(workspace, score_out, frame_rows, "enhance_scores")
        native.check(self.lib.icv_enhance_scores_bf16(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), frames, frame_rows, heads, float(scale),
                                                      float(weight), workspace.data_ptr(), native.ptr(score_out), self._stream()),
                     "icv_enhance_scores_bf16")

    def enhance_apply(self, att, workspace, frames: int, frame_rows: int, heads: int, weight: float, score_out):
        """att bf16 [rows, d] (row stride allowed) <- bf16(f32(att) * E) in place, E = max(1, (frames + weight) * mean) from the partial
        sums ``enhance_scores`` left in ``workspace``, added up in every block in one fixed order; E -> ``score_out`` (f32, one element)
        (icv_enhance_apply_bf16)."""
        _chk(att, BF16, "enhance_apply.att"); _chk(workspace, F32, "enhance_apply.workspace")
        if att.dim() != 2 or att.shape[0] == 0 or att.shape[1] % 8 or att.stride(0) % 8 or att.data_ptr() % 16:
            raise ValueError(f"enhance_apply: att must be [rows > 0, d % 8 == 0] with a row stride that is a multiple of 8 and 16-byte-aligned "
                             f"rows, got {tuple(att.shape)}")
        if not 2 <= frames <= 32:
            raise ValueError(f"enhance_apply: needs 2 <= frames <= 32, got {frames}")
        if score_out is None:
            raise ValueError("enhance_apply: score_out must be an f32 tensor of one element")
        self._enhance_buffers(workspace, score_out, frame_rows, "enhance_apply")
        native.check(self.lib.icv_enhance_apply_bf16(att.data_ptr(), att.stride(0), att.shape[0], att.shape[1], workspace.data_ptr(), frames,
                                                     frame_rows, heads, float(weight), score_out.data_ptr(), self._stream()),
                     "icv_enhance_apply_bf16")

    @staticmethod
    def _enhance_buffers(workspace, score_out, frame_rows, who):
        if not 0 < frame_rows <= native.ENHANCE_WORKSPACE_FLOATS or workspace.numel() < frame_rows or not workspace.is_contiguous():
            raise ValueError(f"{who}: workspace must hold one contiguous float per position ({frame_rows}; at most "
                             f"{native.ENHANCE_WORKSPACE_FLOATS} positions per frame)")
        if score_out is not None:
            _chk(score_out, F32, f"{who}.score_out")
            if score_out.numel() != 1:
                raise ValueError(f"{who}: score_out must be an f32 tensor of one element")

    # ---- EasyCache step skipping (easycache.py) ---------------------------------------
    def l1_change(self, a, b, workspace, out2, update_b=False):
        """out2[0] = sum|a - b|, out2[1] = sum|a| in fp64 over a, b f32 [rows, cols] (row strides allowed; a latent goes in as one
        row); with ``update_b`` also b <- a in the same pass (icv_l1_change_f64: two launches, fixed summation order, no atomics, no
        host read).  workspace: f64 [ICV_L1_CHANGE_WORKSPACE_DOUBLES]; out2: f64, two contiguous elements outside the workspace."""
        _chk(a, F32, "l1_change.a"); _chk(b, F32, "l1_change.b")
        _chk(workspace, torch.float64, "l1_change.workspace"); _chk(out2, torch.float64, "l1_change.out2")
        if a.dim() != 2 or tuple(a.shape) != tuple(b.shape) or a.numel() == 0:
            raise ValueError(f"l1_change: a and b must be [rows, cols] of one non-empty shape, got {tuple(a.shape)} and {tuple(b.shape)}")
        if workspace.numel() < native.L1_CHANGE_WORKSPACE_DOUBLES or not workspace.is_contiguous() or out2.numel() != 2 or not out2.is_contiguous():
            raise ValueError(f"l1_change: workspace must hold {native.L1_CHANGE_WORKSPACE_DOUBLES} contiguous doubles and out2 two")
        rows, cols = a.shape
        lda, ldb = (a.stride(0), b.stride(0)) if rows > 1 else (cols, cols)
        native.check(self.lib.icv_l1_change_f64(a.data_ptr(), lda, b.data_ptr(), ldb, rows, cols, int(bool(update_b)),
                                                workspace.data_ptr(), out2.data_ptr(), self._stream()), "icv_l1_change_f64")

    def easycache_predict(self, x, x_last, hc_last, hu_last, hc, hu, tok0, n_tok):
        """A skipped step's head outputs: for the local tokens, h = h_last + P(x - x_last) with P the head-output layout of a latent
        (unpatchify_cfg_euler's index map read in the other direction), for hc and - unless hu_last and hu are both None - hu, in ONE
        launch (icv_easycache_predict_f32).  x, x_last f32 [C, T, H8, W8]; the four head tensors f32 [>= n_tok, >= 4*C], one stride."""
        _chk(x, F32, "easycache_predict.x"); _chk(x_last, F32, "easycache_predict.x_last")
        if x.dim() != 4 or tuple(x_last.shape) != tuple(x.shape) or not x.is_contiguous() or not x_last.is_contiguous():
            raise ValueError(f"easycache_predict: x and x_last must be contiguous [C, T, H8, W8] latents of one shape, got {tuple(x.shape)} and {tuple(x_last.shape)}")
        if (hu_last is None) != (hu is None):
            raise ValueError("easycache_predict: hu_last and hu must be given together")
        C = x.shape[0]
        heads = [t for t in (hc_last, hu_last, hc, hu) if t is not None]
        for t in heads:
            _chk(t, F32, "easycache_predict.head")
            if t.dim() != 2 or t.shape[0] < n_tok or t.shape[1] < 4 * C or t.stride(0) != hc.stride(0):
                raise ValueError("easycache_predict: head outputs have fewer rows than n_tok or fewer than 4*C columns (or differ in row stride)")
        if len({t.data_ptr() for t in heads}) != len(heads):
            raise ValueError("easycache_predict: the head outputs must be buffers of their own")
        C, T, H8, W8 = x.shape
        native.check(self.lib.icv_easycache_predict_f32(x.data_ptr(), x_last.data_ptr(), hc_last.data_ptr(), native.ptr(hu_last), hc.data_ptr(),
                                                        native.ptr(hu), hc.stride(0), C, T, H8, W8, tok0, n_tok, self._stream()),
                     "icv_easycache_predict_f32")

    def read_doubles(self, t):
        """The values of a small f64 device tensor (at most 8 doubles = 64 bytes) as Python floats: ONE blocking read on the current
        stream - EasyCache's per-step sums, the only data-dependent loop control of the denoising loop."""
        _chk(t, torch.float64, "read_doubles.t")
        if t.numel() > 8 or not t.is_contiguous():
            raise ValueError(f"read_doubles: at most 8 contiguous doubles, got {tuple(t.shape)}")
        return t.cpu().tolist()

    def unpatchify_cfg_euler_window(self, latent_next, hc, hu, cfg_scale, dsigma, frame_coef, frame0, tok0, n_tok, round_bf16=False):
        """Sliding temporal windows (sliding_window.py): latent_next[:, frame0 + f] += frame_coef[f] * (CFG(hc, hu) * dsigma) for the
        window-local tokens [tok0, tok0 + n_tok); hc / hu f32 [n_tok, 4*C], frame_coef f32 [frames of the window] on the device."""
        _chk(latent_next, F32, "euler_window.latent"); _chk(hc, F32, "euler_window.hc"); _chk(frame_coef, F32, "euler_window.frame_coef")
        assert latent_next.is_contiguous() and frame_coef.is_contiguous()
        C, T, H8, W8 = latent_next.shape
        per_frame = (H8 // 2) * (W8 // 2)
        if hc.shape[0] < n_tok or (hu is not None and (hu.shape[0] < n_tok or hu.stride(0) != hc.stride(0))):
            raise ValueError("unpatchify_cfg_euler_window: head outputs have fewer rows than n_tok (or differ in row stride)")
        if frame_coef.numel() * per_frame < tok0 + n_tok:
            raise ValueError(f"unpatchify_cfg_euler_window: {frame_coef.numel()} frame coefficients do not cover window tokens [{tok0}, {tok0 + n_tok})")
        native.check(self.lib.icv_unpatchify_cfg_euler_window(
            latent_next.data_ptr(), hc.data_ptr(), native.ptr(hu), hc.stride(0), cfg_scale, dsigma, frame_coef.data_ptr(), frame0,
            C, T, H8, W8, tok0, n_tok, int(bool(round_bf16)), self._stream()), "icv_unpatchify_cfg_euler_window")

    def cast_bf16(self, src, out):
        _chk(src, F32, "cast.src"); _chk(out, BF16, "cast.out")
        assert src.is_contiguous() and out.is_contiguous() and src.numel() == out.numel()
        native.check(self.lib.icv_cast_f32_to_bf16(src.data_ptr(), out.data_ptr(), src.numel(),
                                                   self._stream()), "icv_cast_f32_to_bf16")

    # ---- TeaCache step skipping (teacache.py) ------------------------------------------------------
    def sub_rows(self, x, r):
        """r = x - r in place; x, r f32 [rows, d] (row strides allowed: halves of the pair engine, shard views)."""
        _chk(x, F32, "sub_rows.x"); _chk(r, F32, "sub_rows.r")
        if x.dim() != 2 or tuple(x.shape) != tuple(r.shape):
            raise ValueError(f"sub_rows: shapes {tuple(x.shape)} and {tuple(r.shape)} differ (or are not [rows, d])")
        rows, d = r.shape
        native.check(self.lib.icv_sub_rows_f32(x.data_ptr(), x.stride(0), r.data_ptr(), r.stride(0), rows, d,
                                               self._stream()), "icv_sub_rows_f32")

    def rel_l1_steps(self, table, out):
        """table f32 [N, cols] (one t_mod row per step) -> out f32 [N]: out[i] = mean|t_i - t_{i-1}| / mean|t_{i-1}|, out[0] = 0."""
        _chk(table, F32, "rel_l1.table"); _chk(out, F32, "rel_l1.out")
        if table.dim() != 2:
            raise ValueError(f"rel_l1_steps: table must be [N, cols], got {tuple(table.shape)}")
        n, cols = table.shape
        assert out.is_contiguous() and out.numel() == n
        native.check(self.lib.icv_rel_l1_steps_f32(table.data_ptr(), n, cols, table.stride(0), out.data_ptr(),
                                                   self._stream()), "icv_rel_l1_steps_f32")

    # ---- LoRA merge (lora.py) --------------------------------------------------------
    def lora_merge(self, w, up, down_t, alpha: float):
        """w += alpha * up @ down_t.T in place, one bf16 rounding: w bf16 [N, K] (a row range of a taller matrix is fine),
        up bf16 [N, R], down_t bf16 [K, R]; shape / alignment contract of icv_lora_merge_bf16 (checked there, before any launch)."""
        _chk(w, BF16, "lora_merge.w"); _chk(up, BF16, "lora_merge.up"); _chk(down_t, BF16, "lora_merge.down_t")
        if w.dim() != 2 or up.dim() != 2 or down_t.dim() != 2:
            raise ValueError("lora_merge: w, up and down_t must be matrices")
        N, K = w.shape
        R = up.shape[1]
        if tuple(up.shape) != (N, R) or tuple(down_t.shape) != (K, R):
            raise ValueError(f"lora_merge: w {tuple(w.shape)} needs up [N, R] and down_t [K, R], got {tuple(up.shape)} and {tuple(down_t.shape)}")
        native.check(self.lib.icv_lora_merge_bf16(w.data_ptr(), w.stride(0), up.data_ptr(), up.stride(0), down_t.data_ptr(),
                                                  down_t.stride(0), N, K, R, float(alpha), self._stream()), "icv_lora_merge_bf16")

    # ---- video-to-video start latent (v2v.py) ----------------------------------------
    def add_noise(self, x0, noise, out, sigma: float, round_bf16=False):
        """out = (1 - sigma) * x0 + sigma * noise, elementwise f32 (icv_add_noise_f32: no fused multiply-add; with round_bf16 both
        products and the sum are rounded to bf16).  ``out`` may be ``noise`` or ``x0`` itself; any other overlap is the caller's error."""
        _chk(x0, F32, "add_noise.x0"); _chk(noise, F32, "add_noise.noise"); _chk(out, F32, "add_noise.out")
        if tuple(x0.shape) != tuple(noise.shape) or tuple(out.shape) != tuple(noise.shape):
            raise ValueError(f"add_noise: x0 {tuple(x0.shape)}, noise {tuple(noise.shape)} and out {tuple(out.shape)} must have one shape")
        assert x0.is_contiguous() and noise.is_contiguous() and out.is_contiguous()
        native.check(self.lib.icv_add_noise_f32(x0.data_ptr(), noise.data_ptr(), out.data_ptr(), out.numel(), float(sigma),
                                                int(bool(round_bf16)), self._stream()), "icv_add_noise_f32")

    # ---- coarse-to-fine sampling (coarse.py) -------------------------------------------
    def latent_resize_noise(self, x0, noise_out, sigma: float, round_bf16=False):
        """noise_out <- (1 - sigma) * up(x0) + sigma * noise_out in ONE launch (icv_latent_resize_noise_f32): x0 f32 [..., h_in, w_in],
        noise_out f32 [..., h_out, w_out] with the same leading dimensions, h_out >= h_in and w_out >= w_in; up is the bilinear
        resize of every plane with half-pixel centres, no fused multiply-add; with round_bf16 the two products and the sum of the
        noising are rounded to bf16.  x0 is read only and must not overlap noise_out."""
        _chk(x0, F32, "latent_resize_noise.x0"); _chk(noise_out, F32, "latent_resize_noise.noise_out")
        if x0.dim() < 2 or x0.dim() != noise_out.dim() or tuple(x0.shape[:-2]) != tuple(noise_out.shape[:-2]):
            raise ValueError(f"latent_resize_noise: x0 {tuple(x0.shape)} and noise_out {tuple(noise_out.shape)} must be [..., h, w] with the same leading dimensions")
        (h_in, w_in), (h_out, w_out) = x0.shape[-2:], noise_out.shape[-2:]
        if h_out < h_in or w_out < w_in:
            raise ValueError(f"latent_resize_noise: the output plane {(h_out, w_out)} must be at least the input plane {(h_in, w_in)} in both dimensions")
        assert x0.is_contiguous() and noise_out.is_contiguous()
        planes = noise_out.numel() // max(h_out * w_out, 1)
        native.check(self.lib.icv_latent_resize_noise_f32(x0.data_ptr(), noise_out.data_ptr(), planes, h_in, w_in, h_out, w_out, float(sigma),
                                                          int(bool(round_bf16)), self._stream()), "icv_latent_resize_noise_f32")

    # ---- regenerating part of a clip (inpaint.py) -------------------------------------
    def latent_keep_mask(self, mask_u8, keep_u8):
        """mask u8 [N, H, W] (non-zero = regenerate) -> keep u8 [(N - 1) / 4 + 1, H / 8, W / 8]: 1 where every mask byte of the
        cell's stride footprint is 0 (icv_latent_keep_mask_u8)."""
        _chk(mask_u8, torch.uint8, "latent_keep_mask.mask"); _chk(keep_u8, torch.uint8, "latent_keep_mask.keep")
        if mask_u8.dim() != 3 or mask_u8.shape[0] % 4 != 1 or mask_u8.shape[1] % 16 or mask_u8.shape[2] % 16:
            raise ValueError(f"latent_keep_mask: mask must be [4k + 1, H, W] with H and W multiples of 16, got {tuple(mask_u8.shape)}")
        N, H, W = mask_u8.shape
        if tuple(keep_u8.shape) != ((N - 1) // 4 + 1, H // 8, W // 8):
            raise ValueError(f"latent_keep_mask: keep must be {((N - 1) // 4 + 1, H // 8, W // 8)} for a mask of {(N, H, W)}, got {tuple(keep_u8.shape)}")
        assert mask_u8.is_contiguous() and keep_u8.is_contiguous()
        native.check(self.lib.icv_latent_keep_mask_u8(mask_u8.data_ptr(), keep_u8.data_ptr(), N, H, W, self._stream()), "icv_latent_keep_mask_u8")

    def pin_known(self, latent, x0, noise, keep, sigma_next: float, x_hat=None, sigma_cur: float = 0.0, m_new=None, round_bf16=False):
        """Where keep != 0: latent = (1 - sigma_next) * x0 + sigma_next * noise in add_noise's arithmetic, x_hat (if given) the same
        at sigma_cur, m_new (if given) = x0; other elements are not written (icv_pin_known_f32).  latent, x0, noise, x_hat, m_new
        f32 [C, ...] of one shape, keep u8 of that shape without the channel dimension."""
        _chk(latent, F32, "pin_known.latent"); _chk(x0, F32, "pin_known.x0"); _chk(noise, F32, "pin_known.noise")
        _chk(keep, torch.uint8, "pin_known.keep")
        if x_hat is not None:
            _chk(x_hat, F32, "pin_known.x_hat")
        if m_new is not None:
            _chk(m_new, F32, "pin_known.m_new")
        shape = tuple(latent.shape)
        if len(shape) < 1 or any(tuple(t.shape) != shape for t in (x0, noise, x_hat, m_new) if t is not None):
            raise ValueError(f"pin_known: latent {shape}, x0 {tuple(x0.shape)}, noise {tuple(noise.shape)}, x_hat and m_new must have one shape")
        if tuple(keep.shape) != shape[1:]:
            raise ValueError(f"pin_known: keep must be {shape[1:]} for a latent of {shape}, got {tuple(keep.shape)}")
        assert all(t.is_contiguous() for t in (latent, x0, noise, keep, x_hat, m_new) if t is not None)
        native.check(self.lib.icv_pin_known_f32(latent.data_ptr(), native.ptr(x_hat), native.ptr(m_new), x0.data_ptr(), noise.data_ptr(),
                                                keep.data_ptr(), shape[0], keep.numel(), float(sigma_next), float(sigma_cur),
                                                int(bool(round_bf16)), self._stream()), "icv_pin_known_f32")
