"""Thin torch-tensor wrappers over the C ABI (include/sd_amd.h).  torch is used only for device
memory and the current HIP stream; every computation happens inside libsdamd.so."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import lib as L

_DT = {torch.float32: L.F32, torch.bfloat16: L.BF16, torch.float16: L.F16}
COMPUTE_DTYPES = tuple(_DT)


def dt_code(dtype: torch.dtype) -> int:
    try:
        return _DT[dtype]
    except KeyError:
        raise L.SdaError(f"unsupported compute dtype {dtype}; use torch.float32, torch.bfloat16 or torch.float16")


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


# The stream every launch goes to = torch's current stream of the current device.  torch.cuda.current_stream().cuda_stream builds
# a Stream object through three Python layers (4-5 us; ~165 launches per step); the two C entry points below are what it ends in.
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def _st():
    if _raw_stream is not None and _cur_device is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


def stream_create_cumask(words) -> int:
    """A HIP stream restricted to the CUs set in `words` (32 CUs per word); returns the hipStream_t as an integer for
    torch.cuda.ExternalStream.  Created in this process; kept in _CREATED_STREAMS until stream_destroy_all()."""
    arr = (C.c_uint32 * len(words))(*[int(w) & 0xFFFFFFFF for w in words])
    out = C.c_void_p()
    L.check(L.load().sda_stream_create_cumask(arr, len(words), C.byref(out)), "stream_create_cumask")
    _CREATED_STREAMS.append(int(out.value))
    return int(out.value)


def stream_create_priority(priority: int) -> int:
    """A non-blocking HIP stream of `priority` (-1 high, 0 normal, 1 LOW: the last is below anything torch's stream pool
    hands out); returns the hipStream_t as an integer for torch.cuda.ExternalStream (destroyed by stream_destroy_all())."""
    out = C.c_void_p()
    L.check(L.load().sda_stream_create_priority(int(priority), C.byref(out)), "stream_create_priority")
    _CREATED_STREAMS.append(int(out.value))
    return int(out.value)


_CREATED_STREAMS = []       # hipStream_t handles made through the C ABI (torch's ExternalStream does not own them)


def stream_destroy_all():
    """Destroy every stream stream_create_cumask / stream_create_priority handed out (call once the ExternalStreams that
    wrap them are no longer used: end of a run).  Idempotent."""
    lib = L.load()
    while _CREATED_STREAMS:
        lib.sda_stream_destroy(C.c_void_p(_CREATED_STREAMS.pop()))


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise L.SdaError("libsdamd kernels need device tensors (no CPU fallback)")


def _need_values(t, dtype, count: int, msg: str, *said):
    """`t` (None passes, as in _need_cuda) holds `count` contiguous values of `dtype` on the device, or SdaError(msg.format(*said))."""
    if t is not None and (t.dtype != dtype or not t.is_contiguous() or t.numel() < count or not t.is_cuda):
        raise L.SdaError(msg.format(*said))


def _need_fp32_rows(t, rows: int, C: int, msg: str):
    """`t` is `rows` fp32 rows, any pitch, of at least C unit-stride columns, or SdaError(msg)."""
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] < rows or t.shape[1] < C or t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        raise L.SdaError(msg)


def upload_small(array, device) -> torch.Tensor:
    """Host numpy array -> new device tensor without a memcpy (payload travels in kernel arguments)."""
    array = np.ascontiguousarray(array)
    nbytes = array.nbytes
    padded = (nbytes + 3) // 4 * 4
    raw = np.zeros(padded, dtype=np.uint8)
    raw[:nbytes] = array.view(np.uint8).reshape(-1)
    out = torch.empty(padded, dtype=torch.uint8, device=device)
    L.check(L.load().sda_upload_words(out.data_ptr(), raw.ctypes.data, padded // 4, _st()), "upload_words")
    tdt = torch.from_numpy(np.empty(0, dtype=array.dtype)).dtype
    return out[:nbytes].view(tdt).reshape(array.shape)


class UploadCache:
    """Small host->device tables (index tables, masks, descriptor tables) keyed by CONTENT.  An upload from
    pageable memory costs the stream ~0.2 ms of idle time (staging round trip when the stream reaches it), and
    most of these tables repeat (one dropout mask per sensor; descriptor tables; recurring batches), so a hit
    returns the device tensor uploaded earlier and nothing is enqueued."""

    def __init__(self, capacity: int = 1024, upload=None):
        import collections
        self.capacity = capacity
        self.items = collections.OrderedDict()
        self._upload = upload or upload_small     # (array, device) -> tensor; the keying and eviction rules do not depend on it

    def upload(self, key, array, device) -> torch.Tensor:
        array = np.ascontiguousarray(array)
        k = (key, str(array.dtype), array.shape, array.tobytes(), str(device))
        hit = self.items.get(k)
        if hit is not None:
            self.items.move_to_end(k)
            return hit
        dev = self._upload(array, device)
        self.items[k] = dev
        if len(self.items) > self.capacity:
            self.items.popitem(last=False)
        return dev


UPLOADER = UploadCache()


def new_rows(B: int, T: int, Cp: int, dtype, device) -> torch.Tensor:
    """Zero-initialised RL buffer: (rows_alloc, Cp)."""
    return torch.zeros((L.rows_alloc(B, T), Cp), dtype=dtype, device=device)


def new_rows_uninit(B: int, T: int, Cp: int, dtype, device) -> torch.Tensor:
    """RL buffer whose VALID rows are left uninitialised (the producing kernel writes all of them); the pad rows in
    front of every sample and the slack behind the last one are zeroed (two small fills instead of a full memset)."""
    buf = torch.empty((L.rows_alloc(B, T), Cp), dtype=dtype, device=device)
    return zero_pad_rows(buf, B, T)


def zero_pad_rows(buf: torch.Tensor, B: int, T: int) -> torch.Tensor:
    """Zero the pad rows in front of every sample and the slack behind the last one of an RL buffer (one small launch)."""
    L.check(L.load().sda_zero_pad_rows(_p(buf), B, T, buf.shape[1], dt_code(buf.dtype), _st()), "zero_pad_rows")
    return buf


def zeros(shape, dtype, device) -> torch.Tensor:
    """A fresh zero tensor filled by sda_fill_zero (no framework fill kernel inside the step)."""
    out = torch.empty(shape, dtype=dtype, device=device)
    if out.numel():
        L.check(L.load().sda_fill_zero(out.data_ptr(), out.numel() * out.element_size(), _st()), "fill_zero")
    return out


def fill_zero_(t: torch.Tensor) -> torch.Tensor:
    """Zero a contiguous device tensor in place (sda_fill_zero)."""
    if not t.is_contiguous():
        raise L.SdaError("fill_zero_: a contiguous tensor")
    if t.numel():
        L.check(L.load().sda_fill_zero(t.data_ptr(), t.numel() * t.element_size(), _st()), "fill_zero")
    return t


def gather_samples(table: torch.Tensor, idx: torch.Tensor, B: int, T: int) -> torch.Tensor:
    """table: row-layout buffer holding N samples back to back ((N * Tp [+ slack], Cp), pad rows zero); idx: B int64 sample
    indices on the device.  Returns a fresh row-layout buffer (rows_alloc(B, T), Cp) whose sample b is table sample idx[b]."""
    _need_cuda(table, idx)
    if idx.dtype != torch.int64 or idx.numel() != B:
        raise L.SdaError("gather_samples: idx must hold B int64 indices")
    Cp = table.shape[1]
    out = new_rows_uninit(B, T, Cp, table.dtype, table.device)
    L.check(L.load().sda_gather_samples(_p(table), _p(idx), _p(out), B, L.rows_tp(T) * Cp * table.element_size(), _st()), "gather_samples")
    return out


def gather_windows(table: torch.Tensor, starts: torch.Tensor, idx: torch.Tensor, B: int, T: int) -> torch.Tensor:
    """table: (L, Cp) plain rows (retrieval.WindowBank.table, Cp a multiple of 64, channel padding zero); starts: M int32 table
    rows on the device; idx: B int64 candidates on the device (any order, duplicates allowed).  Returns a fresh row-layout buffer
    (rows_alloc(B, T), Cp) whose sample b is the T table rows from starts[idx[b]] on.  ONE launch writes all of it, pad rows and
    slack included; a candidate outside [0, M) or a window that leaves the table comes back as zeros."""
    _need_cuda(table, starts, idx)
    if idx.dtype != torch.int64 or idx.numel() != B or not idx.is_contiguous():
        raise L.SdaError("gather_windows: idx must hold B int64 indices")
    if starts.dtype != torch.int32 or starts.dim() != 1 or not starts.is_contiguous() or starts.numel() < 1:
        raise L.SdaError("gather_windows: starts must be a contiguous one-dimensional int32 tensor of at least one table row")
    if table.dim() != 2 or not table.is_contiguous() or table.dtype not in COMPUTE_DTYPES:
        raise L.SdaError("gather_windows: table must be a contiguous (L, Cp) tensor of float32, bfloat16 or float16 rows")
    if table.device != starts.device or table.device != idx.device:
        raise L.SdaError(f"gather_windows: table on {table.device}, starts on {starts.device}, idx on {idx.device}")
    Cp = table.shape[1]
    out = torch.empty((L.rows_alloc(B, T), Cp), dtype=table.dtype, device=table.device)      # the kernel writes all of it
    L.check(L.load().sda_gather_windows(_p(table), table.shape[0], _p(starts), starts.numel(), _p(idx), _p(out), B, T,
                                        Cp * table.element_size(), _st()), "gather_windows")
    return out


def clip_merge_rows(allp: torch.Tensor):
    """allp: the all-gathered (world, 3, Bg) fp32 table of per-rank (row max, row sum exp, positive's logit) -> (lse, diag)."""
    world, k, Bg = allp.shape
    if k != 3 or allp.dtype != torch.float32 or not allp.is_contiguous():
        raise L.SdaError("clip_merge_rows: a contiguous fp32 (world, 3, B_global) table")
    out = torch.empty((2, Bg), dtype=torch.float32, device=allp.device)
    L.check(L.load().sda_clip_merge_rows(_p(allp), world, Bg, _p(out[0]), _p(out[1]), _st()), "clip_merge_rows")
    return out[0], out[1]


def scalar_mul(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a * b[0] for small fp32 device tensors (a: n elements, b: one)."""
    out = torch.empty_like(a)
    L.check(L.load().sda_scalar_mul(_p(a), _p(b), _p(out), a.numel(), _st()), "scalar_mul")
    return out


def rows_view(buf: torch.Tensor, B: int, C: int, T: int) -> torch.Tensor:
    """(B, C, T) strided view of an RL buffer (zero copy): element (b, c, t) = buf[b*Tp + PAD + t, c]."""
    Tp, Cp = L.rows_tp(T), buf.shape[1]
    return buf.as_strided((B, C, T), (Tp * Cp, 1, Cp), L.ROW_PAD * Cp)


def rows_base(t: torch.Tensor, B: int, Cc: int, T: int, dtype) -> Optional[torch.Tensor]:
    """The inverse of rows_view: if `t` is a (B, C, T) view of `dtype` laid out exactly like rows_view(...) of an RL buffer,
    that buffer as a (rows_alloc, Cp) tensor sharing its storage (zero copy); else None."""
    if t.dtype != dtype or not t.is_cuda or t.dim() != 3:
        return None
    Cp, rows = L.pad_channels(Cc), L.rows_alloc(B, T)
    if tuple(t.stride()) != (L.rows_tp(T) * Cp, 1, Cp) or t.storage_offset() != L.ROW_PAD * Cp:
        return None
    if t.untyped_storage().nbytes() < rows * Cp * t.element_size():
        return None
    return t.detach().as_strided((rows, Cp), (Cp, 1), 0)


def rows_of(t: torch.Tensor, Cc: int, dtype, alloc=new_rows):
    """(RL buffer of `dtype` holding the (B, C, T) device tensor `t`, was_view): the buffer behind a rows view made by this
    package (zero copy, True); else `t` packed into the buffer `alloc(B, T, Cp, dtype, device)` hands out (new_rows,
    new_rows_uninit or a caller's pool; not called for a view), and False."""
    B, _, T = t.shape
    base = rows_base(t, B, Cc, T, dtype)
    if base is not None:
        return base, True
    return pack_rows(t.detach(), alloc(B, T, L.pad_channels(Cc), dtype, t.device)), False


def pack_rows(src: torch.Tensor, dst: torch.Tensor, ones_channel: Optional[int] = None) -> torch.Tensor:
    """(B, C, T) device tensor -> RL buffer `dst` of its own dtype in one pass; with `ones_channel` that padding channel is 1 on
    every valid row.  Valid rows and their channel padding are written, pad rows are not: `dst` comes from new_rows /
    new_rows_uninit.  An fp32 source takes sda_pack_rows / sda_pack_rows_ones, a bf16 / fp16 one sda_pack_rows_typed (widened
    in registers: no fp32 copy).  A source that is not contiguous is made so first."""
    _need_cuda(src, dst)
    if src.dim() != 3:
        raise L.SdaError("pack_rows: src must be a (B, C, T) tensor")
    B, Cc, T = src.shape
    if dst.dim() != 2 or not dst.is_contiguous() or dst.shape[0] < L.rows_alloc(B, T):
        raise L.SdaError("pack_rows: dst must be a row-layout buffer for (B, T)")
    if src.dtype not in _DT or (ones_channel is not None and src.dtype != torch.float32):
        # no entry point packs a 16-bit source WITH a ones channel (the composed SubjectBlock fed a 16-bit X): that one, and a
        # dtype the kernels do not read, go through an fp32 copy
        src = src.float()
    src = src.contiguous()
    lib, Cp, dt = L.load(), dst.shape[1], dt_code(dst.dtype)
    if ones_channel is not None:
        L.check(lib.sda_pack_rows_ones(_p(src), _p(dst), B, Cc, T, Cp, ones_channel, dt, _st()), "pack_rows_ones")
    elif src.dtype == torch.float32:
        L.check(lib.sda_pack_rows(_p(src), _p(dst), B, Cc, T, Cp, dt, _st()), "pack_rows")
    else:
        L.check(lib.sda_pack_rows_typed(_p(src), _p(dst), B, Cc, T, Cp, dt_code(src.dtype), dt, _st()), "pack_rows_typed")
    return dst


def unpack_rows(src: torch.Tensor, B: int, Cc: int, T: int, dtype=torch.float32) -> torch.Tensor:
    """RL buffer -> a fresh contiguous (B, C, T) tensor of `dtype` (fp32 / bf16 / fp16), one HBM pass."""
    _need_cuda(src)
    out = torch.empty((B, Cc, T), dtype=dtype, device=src.device)
    L.check(L.load().sda_unpack_rows_typed(_p(src), _p(out), B, Cc, T, src.shape[1], dt_code(src.dtype), dt_code(dtype), _st()),
            "unpack_rows")
    return out


def input_grad(G: torch.Tensor, W: torch.Tensor, widx: Optional[torch.Tensor], B: int, Cc: int, T: int, dtype) -> torch.Tensor:
    """dX[b][c][t] = sum_d W[w_b][d][c] G[row(b, t)][d] (sda_input_grad): G a row-layout buffer of the compute dtype, W the
    (nW, 1, Kp, Cp) or (nW, Kp, Cp) matrix the forward applied, widx B device int32 indices (None: one matrix).  Returns a fresh
    contiguous (B, C, T) tensor of `dtype` (fp32 / bf16 / fp16)."""
    _need_cuda(G, W)
    Wv = W.reshape(W.shape[0], W.shape[-2], W.shape[-1]) if W.dim() == 4 and W.shape[1] == 1 else W
    if Wv.dim() != 3 or not Wv.is_contiguous() or Wv.dtype != G.dtype:
        raise L.SdaError("input_grad: W must be a contiguous (nW, Kp, Cp) tensor of G's dtype")
    if G.dim() != 2 or not G.is_contiguous() or G.shape[0] < L.rows_alloc(B, T) or G.shape[1] < Wv.shape[1]:
        raise L.SdaError("input_grad: G must be a row-layout buffer at least Kp channels wide")
    if widx is not None and (widx.dtype != torch.int32 or widx.numel() != B or not widx.is_cuda):
        raise L.SdaError("input_grad: widx must hold B int32 indices on the device")
    out = torch.empty((B, Cc, T), dtype=dtype, device=G.device)
    L.check(L.load().sda_input_grad(_p(G), G.shape[1], _p(Wv), _p(widx), Wv.shape[0], Wv.shape[1], Wv.shape[2], B, Cc, T,
                                    dt_code(G.dtype), _p(out), dt_code(dtype), _st()), "input_grad")
    return out


def rows_sumsq(x: torch.Tensor, B: int, row_elems: int, pitch: int) -> torch.Tensor:
    out = torch.empty(B, dtype=torch.float32, device=x.device)
    scratch = torch.empty(B * 64, dtype=torch.float32, device=x.device)
    L.check(L.load().sda_rows_sumsq(_p(x), _p(out), _p(scratch), B, row_elems, pitch, dt_code(x.dtype), _st()), "rows_sumsq")
    return out


def _mse_operand(t: torch.Tensor, B: int, F: int, T: int):
    """(pointer, cp, dtype code) of an MSE operand: a row-layout buffer (rows_alloc, Cp) or a contiguous (B, F, T) tensor."""
    _need_cuda(t)
    if t.dim() == 2 and t.shape[0] >= L.rows_alloc(B, T) and t.is_contiguous():
        return _p(t), t.shape[1], dt_code(t.dtype)
    if tuple(t.shape) == (B, F, T) and t.is_contiguous():
        return _p(t), 0, dt_code(t.dtype)
    raise L.SdaError(f"mse: operand of shape {tuple(t.shape)} is neither a row-layout buffer nor a contiguous {(B, F, T)} tensor")


def mse_forward(z: torch.Tensor, y: torch.Tensor, B: int, F: int, T: int, b_div: int) -> torch.Tensor:
    """sum (y - z)^2 / b_div as a 0-dim fp32 device tensor; z, y: row-layout buffers or contiguous (B, F, T) tensors."""
    zo, yo = _mse_operand(z, B, F, T), _mse_operand(y, B, F, T)
    out = torch.empty((), dtype=torch.float32, device=z.device)
    scratch = torch.empty(L.MSE_PARTIALS, dtype=torch.float64, device=z.device)
    L.check(L.load().sda_mse_forward(*zo, *yo, B, F, T, b_div, _p(scratch), _p(out), _st()), "mse_forward")
    return out


def mse_backward(z: torch.Tensor, y: torch.Tensor, B: int, F: int, T: int, b_div: int, dloss: torch.Tensor,
                 dz: Optional[torch.Tensor], dy: Optional[torch.Tensor]):
    """dz = 2 (dloss / b_div) (z - y) in z's form and dtype, dy = -that in y's form and dtype (either may be None); dloss: one fp32
    element on the device.  A row-layout output needs zeroed pad rows and slack (new_rows_uninit)."""
    zo, yo = _mse_operand(z, B, F, T), _mse_operand(y, B, F, T)
    for out, src in ((dz, z), (dy, y)):
        if out is not None and (out.shape != src.shape or out.dtype != src.dtype or not out.is_contiguous()):
            raise L.SdaError("mse_backward: a gradient must have its operand's shape, dtype and layout")
    L.check(L.load().sda_mse_backward(*zo, *yo, B, F, T, b_div, _p(dloss), _p(dz), _p(dy), _st()), "mse_backward")


def rows_sumsq_from_row_parts(parts: torch.Tensor, B: int, T: int) -> torch.Tensor:
    """Per-sample sum of squares from the per-row partial sums conv_gemm(row_sumsq=parts) wrote."""
    out = torch.empty(B, dtype=torch.float32, device=parts.device)
    L.check(L.load().sda_rows_sumsq_from_row_parts(_p(parts), parts.shape[1], _p(out), B, T, _st()), "rows_sumsq_from_row_parts")
    return out


def rows_sumsq_from_stats(stats: torch.Tensor, B: int) -> torch.Tensor:
    """Per-sample sum of squares of a conv output from the per-tile statistics its epilogue wrote (plane 1)."""
    out = torch.empty(B, dtype=torch.float32, device=stats.device)
    L.check(L.load().sda_rows_sumsq_from_stats(_p(stats), stats.shape[0] // B, stats.shape[2], _p(out), B, _st()),
            "rows_sumsq_from_stats")
    return out


class _NormCache:
    """Squared norms of RL buffers whose producer already summed them (the encoder's last conv).  An entry is valid only
    while the PRODUCER'S tensor object is alive (a freed buffer's address can be handed to an unrelated tensor), for
    the same storage at the same torch version counter: an in-place torch op on the tensor (or any view of it)
    invalidates it; the producing kernel refreshes it on every forward."""

    def __init__(self):
        self.items = {}

    def put(self, buf: torch.Tensor, sumsq: torch.Tensor):
        import weakref
        if len(self.items) > 16:
            self.items = {k: v for k, v in self.items.items() if v[0]() is not None}
        self.items[buf.data_ptr()] = (weakref.ref(buf), buf._version, buf.shape[0], sumsq)

    def get(self, buf: torch.Tensor, B: int):
        hit = self.items.get(buf.data_ptr())
        if hit is None:
            return None
        owner = hit[0]()
        if (owner is None or owner.data_ptr() != buf.data_ptr() or owner._version != hit[1] or buf._version != hit[1]
                or hit[2] != buf.shape[0] or hit[3].numel() != B):
            return None
        return hit[3]


ROW_NORMS = _NormCache()


def pack_conv_weight(w: torch.Tensor, Cout_p: int, Cin_p: int, dtype, mode: int = 0, glu_half: int = 0,
                     glu_half_p: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """w: (nW, Cout, Cin, KS) or (Cout, Cin, KS) fp32 -> packed operand (nW, KS, rows, cols)."""
    if w.dim() == 3:
        w = w.unsqueeze(0)
    nW, Cout, Cin, KS = w.shape
    w = w.contiguous()
    rows, cols = (Cout_p, Cin_p) if mode == 0 else (Cin_p, Cout_p)
    if out is None:
        out = torch.empty((nW, KS, rows, cols), dtype=dtype, device=w.device)
    L.check(L.load().sda_pack_conv_weight(_p(w), _p(out), nW, Cout, Cin, KS, Cout_p, Cin_p, mode, glu_half, glu_half_p,
                                          dt_code(dtype), _st()), "pack_conv_weight")
    return out


class PackPlan:
    """A fixed list of operand packs (weights -> compute dtype / padded layout, biases -> padded fp32) executed by
    ONE kernel launch.  Sources are the fp32 master parameters (stable addresses), destinations persistent
    buffers; the descriptor table lives on the device and is rebuilt only if a source pointer changes."""

    def __init__(self, dtype, device):
        self.dtype, self.device = dtype, device
        self.items = []          # (key, src tensor, dst tensor, desc fields)
        self.out = {}
        self._table = None
        self._sig = None

    def add_weight(self, key, w, Cout_p, Cin_p, mode=0, glu_half=0, glu_half_p=0, glu_tile=0):
        if w.dim() == 3:
            w = w.unsqueeze(0)
        nW, Cout, Cin, KS = w.shape
        rows, cols = (Cout_p, Cin_p) if mode == 0 else (Cin_p, Cout_p)
        dst = torch.empty((nW, KS, rows, cols), dtype=self.dtype, device=self.device)
        self.items.append((key, w, dst, dict(nW=nW, Cout=Cout, Cin=Cin, KS=KS, Cout_p=Cout_p, Cin_p=Cin_p, mode=mode,
                                             glu_half=glu_half, glu_half_p=glu_half_p, glu_tile=glu_tile, is_vector=0,
                                             total=dst.numel())))
        self.out[key] = dst
        return dst

    def add_vector(self, key, v, Cp, glu_half=0, glu_half_p=0, glu_tile=0):
        dst = torch.empty(Cp, dtype=torch.float32, device=self.device)
        self.items.append((key, v, dst, dict(nW=1, Cout=v.numel(), Cin=1, KS=1, Cout_p=Cp, Cin_p=1, mode=0,
                                             glu_half=glu_half, glu_half_p=glu_half_p, glu_tile=glu_tile, is_vector=1, total=Cp)))
        self.out[key] = dst
        return dst

    def run(self, sources):
        """sources: {key: current fp32 tensor} (same shapes as at add time)."""
        sig = tuple(sources[k].data_ptr() for k, *_ in self.items)
        if sig != self._sig:
            arr = (L.PackDesc * len(self.items))()
            for i, (k, _, dst, f) in enumerate(self.items):
                src = sources[k]
                if not src.is_contiguous():
                    raise L.SdaError(f"pack plan: parameter {k} is not contiguous")
                arr[i].src, arr[i].dst = src.data_ptr(), dst.data_ptr()
                for name, val in f.items():
                    setattr(arr[i], name, val)
            self._table = upload_small(np.frombuffer(bytes(arr), dtype=np.uint8), self.device)
            self._sig = sig
            self._max_total = max(f["total"] for *_, f in self.items)
        L.check(L.load().sda_pack_multi(_p(self._table), len(self.items), self._max_total, dt_code(self.dtype), _st()), "pack_multi")
        return self.out


def reduce_unpack_wgrad(slabs, Cout, Cin, KS, glu_half=0, glu_half_p=0) -> torch.Tensor:
    """slabs (nseg, KS, Cout_p, Cin_p) fp32 -> parameter-layout gradient (Cout, Cin, KS) fp32."""
    out = torch.empty((Cout, Cin, KS), dtype=torch.float32, device=slabs.device)
    L.check(L.load().sda_reduce_unpack_wgrad(_p(slabs), slabs.shape[0], _p(out), Cout, Cin, KS, slabs.shape[2], slabs.shape[3],
                                             glu_half, glu_half_p, _st()), "reduce_unpack_wgrad")
    return out


def pack_vector(v: torch.Tensor, Cp: int, glu_half: int = 0, glu_half_p: int = 0) -> torch.Tensor:
    out = torch.empty(Cp, dtype=torch.float32, device=v.device)
    L.check(L.load().sda_pack_vector(_p(v.contiguous()), _p(out), v.numel(), Cp, glu_half, glu_half_p, _st()), "pack_vector")
    return out


def unpack_conv_wgrad(g: torch.Tensor, nW, Cout, Cin, KS, Cout_p, Cin_p, glu_half=0, glu_half_p=0) -> torch.Tensor:
    out = torch.empty((nW, Cout, Cin, KS), dtype=torch.float32, device=g.device)
    L.check(L.load().sda_unpack_conv_wgrad(_p(g), _p(out), nW, Cout, Cin, KS, Cout_p, Cin_p, glu_half, glu_half_p, _st()),
            "unpack_conv_wgrad")
    return out


def unpack_vector(g: torch.Tensor, Cc: int, glu_half=0, glu_half_p=0) -> torch.Tensor:
    out = torch.empty(Cc, dtype=torch.float32, device=g.device)
    L.check(L.load().sda_unpack_vector(_p(g), _p(out), Cc, g.numel(), glu_half, glu_half_p, _st()), "unpack_vector")
    return out


def param_gemm(A: torch.Tensor, B: torch.Tensor, out: Optional[torch.Tensor] = None, out_dtype=torch.float32) -> torch.Tensor:
    """out[b] = A[b] @ B[b] for fp32 operands of ANY strides — (M, K) @ (K, N), or batched (b, M, K) @ (b, K, N) where a 2-d
    operand is shared by every batch member (views, transposes, slices: nothing is copied or made contiguous).  `out` may be
    a view too (fp32, or the compute dtype: the product is then rounded on the way out); by default a new fp32 tensor."""
    _need_cuda(A, B, out)
    if A.dtype != torch.float32 or B.dtype != torch.float32:
        raise L.SdaError("param_gemm: operands must be fp32")
    batch = A.shape[0] if A.dim() == 3 else (B.shape[0] if B.dim() == 3 else 1)
    M, K = A.shape[-2], A.shape[-1]
    N = B.shape[-1]
    if B.shape[-2] != K or (A.dim() == 3 and B.dim() == 3 and A.shape[0] != B.shape[0]):
        raise L.SdaError(f"param_gemm: shapes {tuple(A.shape)} x {tuple(B.shape)} do not multiply")
    batched = A.dim() == 3 or B.dim() == 3
    if out is None:
        out = torch.empty(((batch, M, N) if batched else (M, N)), dtype=out_dtype, device=A.device)
    if tuple(out.shape[-2:]) != (M, N) or (out.dim() == 3) != batched or (batched and out.shape[0] != batch):
        raise L.SdaError(f"param_gemm: output shape {tuple(out.shape)} does not match ({batch}, {M}, {N})")
    a = L.PgemmArgs()
    a.A, a.B, a.C = A.data_ptr(), B.data_ptr(), out.data_ptr()
    a.M, a.N, a.K, a.batch = M, N, K, batch
    a.a_i, a.a_k, a.a_b = A.stride(-2), A.stride(-1), (A.stride(0) if A.dim() == 3 else 0)
    a.b_k, a.b_j, a.b_b = B.stride(-2), B.stride(-1), (B.stride(0) if B.dim() == 3 else 0)
    a.c_i, a.c_j, a.c_b = out.stride(-2), out.stride(-1), (out.stride(0) if out.dim() == 3 else 0)
    a.c_dtype = dt_code(out.dtype)
    L.check(L.load().sda_param_gemm(C.byref(a), _st()), "param_gemm")
    return out


def copy3d(dst: torch.Tensor, src: torch.Tensor) -> torch.Tensor:
    """dst[...] = src[...] for fp32 views of equal shape (up to 3 dims) and any strides — one small kernel instead of a
    framework copy (column inserts, permuted packs of a parameter)."""
    _need_cuda(dst, src)
    if dst.shape != src.shape or dst.dim() > 3 or dst.dtype != torch.float32 or src.dtype != torch.float32:
        raise L.SdaError("copy3d: fp32 views of equal shape with at most three dimensions")
    pad = 3 - dst.dim()
    n = [1] * pad + list(dst.shape)
    d = [0] * pad + list(dst.stride())
    s_ = [0] * pad + list(src.stride())
    L.check(L.load().sda_copy3d(dst.data_ptr(), d[0], d[1], d[2], src.data_ptr(), s_[0], s_[1], s_[2], n[0], n[1], n[2], _st()), "copy3d")
    return dst


class KernelTimer:
    """Optional HIP-event timing of individual launches on the current stream (bench.py's roofline leg).
    Off by default: `ops.TIMER = KernelTimer()` turns it on, `ops.TIMER = None` off."""

    def __init__(self, families=("conv_gemm",)):
        self.records = []           # (key, algorithmic_flops, start_event, end_event)
        self.families = tuple(families)   # which kernel families get event pairs ("conv_gemm", "wgrad_gemm")

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for key, flops, e0, e1 in self.records:
            n, f, ms = out.get(key, (0, 0.0, 0.0))
            out[key] = (n + 1, f + flops, ms + e0.elapsed_time(e1))
        return out


TIMER: Optional[KernelTimer] = None


def _launch(family: str, label, fn, a, what: str):
    """L.check(fn(&a, stream), what): one GEMM launch.  With the kernel timer on for `family` it runs between two HIP events on the
    CURRENT stream (the side stream in backward), recorded under label() = ((family, dtype name, tile, KS), algorithmic FLOPs)."""
    timed = TIMER is not None and family in TIMER.families
    if timed:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    L.check(fn(C.byref(a), _st()), what)
    if timed:
        e1.record()
        TIMER.records.append((*label(), e0, e1))


def conv_tile_co(Cout_p: int, KS: int = 3, stats: bool = False) -> int:
    """Output-channel tile of sda_conv_gemm's tile-per-workgroup kernels (the kernel timer's labels, linear_rows' ksplit)."""
    return L.load().sda_conv_tile_co(Cout_p, KS, int(stats))


def conv_args(x, w, y, *, B, T, Cin_p, Cout_p, KS, dil, x_pitch, w_pitch, x_rows_limit, dtype, flags=0, bias=None, res=None,
              y_pre=None, widx=None, stats=None, bn_x=None, bn_coef=None, glu_out=None, glu_gate=None,
              x_row0=L.ROW_PAD, x_sample_rows=None, w_rows_limit=None, ksplit=1, partial=None) -> L.ConvArgs:
    """Every field of one sda_conv_gemm descriptor, from device addresses (ints or None), extents, pitches, flags and a dtype code.
    Row layout (the defaults): frame t of sample b is row b * rows_tp(T) + ROW_PAD + t of x, fully padded weights, one K slice.
    Plain matrix / view: the caller gives x_row0, x_sample_rows (from one of the B problems to the next), w_rows_limit, ksplit, partial."""
    return L.ConvArgs(x, w, bias, res, y, y_pre, widx, stats, partial, bn_x, bn_coef, glu_out, glu_gate, B, T, Cin_p, Cout_p, KS, dil,
                      x_pitch, w_pitch, x_row0, L.rows_tp(T) if x_sample_rows is None else x_sample_rows, x_rows_limit,
                      Cout_p if w_rows_limit is None else w_rows_limit, ksplit, flags, dtype)   # (the struct's field order: the cheap way)


def conv_gemm(x, w, y, *, B, T, KS, dil, bias=None, res=None, y_pre=None, widx=None, stats=None, gelu=False,
              alg_dims=None, flags=0, bn_x=None, bn_coef=None, glu_bwd=None, gelu_bwd_u=None, row_sumsq=None):
    """RL conv: x (rows, Cin_p), w (nW, KS, Cout_p, Cin_p) packed, y (rows, Cout_p).
    alg_dims = (Cin, Cout) unpadded, only used to count algorithmic FLOPs when the timer is on.
    gelu_bwd_u (flat 1x1 only, SDA_EPI_GELU_BWD): y = round(conv) * GELU'(gelu_bwd_u), `stats` = per-unit column sums.
    row_sumsq (flat 1x1 only, SDA_EPI_ROW_SUMSQ): float (rows, Cout_p / 128) buffer of per-row partial sums of squares."""
    _need_cuda(x, w, y)
    if gelu_bwd_u is not None:
        if bn_x is not None or gelu_bwd_u.shape != y.shape or stats is None:
            raise L.SdaError("conv_gemm: gelu_bwd_u needs the shape of y and a stats buffer")
        flags |= L.EPI_GELU_BWD
        bn_x = gelu_bwd_u
    if row_sumsq is not None:
        if stats is not None or row_sumsq.dtype != torch.float32 or row_sumsq.shape[0] < B * L.rows_tp(T) \
                or y.shape[1] % 128 or row_sumsq.shape[1] != y.shape[1] // 128:
            raise L.SdaError("conv_gemm: row_sumsq must be float (rows, Cout_p / 128) and excludes stats")
        flags |= L.EPI_ROW_SUMSQ
        stats = row_sumsq
    glu = bool(flags & L.EPI_GLU)        # y (and y_pre = the gate) are half as wide as the conv's output channels
    Cout_p = 2 * y.shape[1] if glu else y.shape[1]
    glu_out, glu_gate = glu_bwd if glu_bwd is not None else (None, None)
    if glu_bwd is not None:              # (out, gate) of the GLU this conv's output is the gradient of: y = [d value | d gate]
        flags |= L.EPI_GLU_BWD
        Cout_p = y.shape[1] // 2
        if glu_out.shape[1] != Cout_p or glu_gate.shape != glu_out.shape or stats is None:
            raise L.SdaError("conv_gemm: glu_bwd needs (out, gate) of the conv's width and a stats buffer")
    if glu and (res is not None or stats is not None or bn_x is not None or (y_pre is not None and y_pre.shape != y.shape)):
        raise L.SdaError("conv_gemm: EPI_GLU takes no residual / statistics and a gate buffer of y's shape")
    if bn_x is not None and gelu_bwd_u is None and (bn_x.shape != y.shape or bn_coef is None or bn_coef.numel() != 4 * y.shape[1] or stats is None):
        raise L.SdaError("conv_gemm: bn_x needs the shape of y, a [4][Cout_p] coefficient table and a stats buffer")
    if w.shape[-1] != x.shape[1] or w.shape[-2] != Cout_p or w.shape[-3] != KS:
        raise L.SdaError(f"conv_gemm: weight {tuple(w.shape)} does not match x {tuple(x.shape)} / y {tuple(y.shape)}")
    if x.shape[0] < L.rows_alloc(B, T) or y.shape[0] < L.rows_alloc(B, T):
        raise L.SdaError("conv_gemm: RL buffers too small for (B, T)")
    a = conv_args(_p(x), _p(w), _p(y), B=B, T=T, Cin_p=x.shape[1], Cout_p=Cout_p, KS=KS, dil=dil, x_pitch=x.shape[1],
                  w_pitch=w.shape[-1], x_rows_limit=x.shape[0], dtype=dt_code(x.dtype), flags=(L.EPI_GELU if gelu else 0) | flags,
                  bias=_p(bias), res=_p(res), y_pre=_p(y_pre), widx=_p(widx), stats=_p(stats), bn_x=_p(bn_x), bn_coef=_p(bn_coef),
                  glu_out=_p(glu_out), glu_gate=_p(glu_gate))
    cin, cout = alg_dims if alg_dims is not None else (x.shape[1], y.shape[1])
    _launch("conv_gemm", lambda: (("conv_gemm", str(x.dtype).replace("torch.", ""), conv_tile_co(Cout_p, KS, stats is not None), KS),
                                  2.0 * B * T * KS * cin * cout), L.load().sda_conv_gemm, a, "conv_gemm")
    return y


def n_t_tiles(T: int) -> int:
    return (T + 127) // 128


def conv_stats_rows(B: int, T: int, KS: int, Cout_p: int, flags: int = 0) -> int:
    """Rows of the per-tile statistics buffer a conv_gemm launch with these parameters writes (-1: it would be refused)."""
    return L.load().sda_conv_stats_rows(B, T, KS, Cout_p, flags)


def conv_kernel(KS: int, Cout_p: int, flags: int, dtype) -> Optional[int]:
    """The kernel conv_gemm routes a convolution to (L.CONV_KERNEL_TILE / _FLAT3 / _FLAT1 / _WIDE), asked of the library that
    routes; None where it refuses these flags for this width or storage type (dtype: torch dtype or dtype code)."""
    k = L.load().sda_conv_kernel(KS, Cout_p, flags, dtype if isinstance(dtype, int) else dt_code(dtype))
    return None if k < 0 else k


# the similarity matmul of 16-bit operands on sim_gemm.hip's 256 x 256 tiles (False: conv_gemm's split-K matrix mode with
# 128 x 128 tiles, which fp32 storage always uses)
SIM_GEMM_TILES256 = True


def k_slab(dtype) -> int:
    return 32 if dtype == torch.float32 else 64      # Elem<E>::SLAB of sda_conv_gemm: a split-K slice is a whole number of these


def splitk_plan(dtype, M: int, N: int, K: int, pitch: int):
    """(tiles256, ksplit) matmul_nt_splitk runs an (M x N) product over K with: sim_gemm.hip's 256 x 256 tiles (16-bit storage) or
    conv_gemm's split-K matrix mode, and the number of K slices."""
    Np = L.pad_channels(N)
    if SIM_GEMM_TILES256 and K <= pitch:
        # 16-bit storage: 256 x 256 output tiles, every operand byte of a K slice through LDS once (csrc/sim_gemm.hip)
        ks = L.load().sda_sim_gemm_ksplit(M, N, K, dt_code(dtype))
        if ks > 0:
            return True, ks
    nslab = K // k_slab(dtype)
    tiles = ((M + 127) // 128) * (Np // splitk_tile_co(Np))      # (the planning count, not conv_tile_co(Np, 1): see splitk_tile_co)
    ksplit = max(1, min(nslab, (512 + tiles - 1) // tiles))
    if nslab <= 64:                 # a short contraction (SpatialAttention's weights: 2048 deep, 270 x 256 outputs): the slab sum
        ksplit = min(ksplit, 16)    # has few threads, each walking every slab — 64 slabs cost 30 us on the step's start chain
    return False, ksplit


def matmul_nt_splitk_into(xm: torch.Tensor, wm: torch.Tensor, M: int, N: int, K: int, pitch: int, tiles256: bool, ksplit: int,
                          partial: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """matmul_nt_splitk with the plan, the K-slice scratch (ksplit * M * pad64(N) floats; unused when ksplit == 1) and the
    destination (M * pad64(N) floats, contiguous) given by the caller.  Any 1 <= ksplit <= K slabs is served; the sum over the
    slices is ordered, so one ksplit always gives the same bits."""
    Np = L.pad_channels(N)
    dst = out if ksplit == 1 else partial
    if tiles256:
        L.check(L.load().sda_sim_gemm(_p(xm), _p(wm), _p(dst), M, N, Np, K, pitch, ksplit, dt_code(xm.dtype), _st()), "sim_gemm")
    else:
        a = conv_args(_p(xm), _p(wm), None, B=1, T=M, Cin_p=K, Cout_p=Np, KS=1, dil=0, x_pitch=pitch, w_pitch=pitch, x_rows_limit=M,
                      dtype=dt_code(xm.dtype), x_row0=0, x_sample_rows=0, w_rows_limit=N, ksplit=ksplit, partial=_p(dst))
        L.check(L.load().sda_conv_gemm(C.byref(a), _st()), "conv_gemm(split-K)")
    if ksplit > 1:
        L.check(L.load().sda_reduce_slabs(_p(partial), _p(out), ksplit, M * Np, _st()), "reduce_slabs")
    return out


def sim_gemm_windows_span(row_elems: int) -> int:
    """Largest start - base_row one sim_gemm_windows launch serves for table rows of `row_elems` elements (asked, not mirrored)."""
    return L.load().sda_sim_gemm_windows_span(row_elems)


def sim_gemm_windows_into(xm: torch.Tensor, x_pitch: int, table: torch.Tensor, starts: torch.Tensor, lo: int, hi: int, row_elems: int,
                          M: int, N: int, K: int, ksplit: int, partial: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out[i][j] = sum_k xm[i][k] * table[starts[j] * row_elems + k] for i < M, j < N (pad64(N) columns per row): matmul_nt_splitk_into
    against N windows of a table of plain rows (sda_sim_gemm_windows + the ordered slab sum).  `starts`: N int32 table rows on
    the device; `lo`, `hi`: their smallest and largest, from the caller's host copy — a chunk whose span hi - lo does not fit the
    kernel's 32-bit offset is refused here, and a window past the table's end too."""
    _need_cuda(xm, table, starts, partial, out)
    _need_values(starts, torch.int32, N, "sim_gemm_windows: starts must hold N contiguous int32 table rows")
    if xm.dtype != table.dtype or not table.is_contiguous():
        raise L.SdaError("sim_gemm_windows: X and a contiguous table of one 16-bit dtype")
    if lo < 0 or hi < lo or hi * row_elems + K > table.numel():
        raise L.SdaError(f"sim_gemm_windows: windows [{lo}, {hi}] x {K} elements leave the table of {table.numel()} elements")
    if hi - lo > sim_gemm_windows_span(row_elems):
        raise L.SdaError(f"sim_gemm_windows: the chunk's windows span table rows {lo} ... {hi}, more than 4 GB (add candidates in "
                         "time order, or lower scratch_bytes for smaller chunks)")
    Np = L.pad_channels(N)
    _need_values(out, torch.float32, M * Np, "sim_gemm_windows: out must hold M * pad64(N) contiguous fp32 values")
    if ksplit > 1:
        _need_values(partial, torch.float32, ksplit * M * Np, "sim_gemm_windows: partial must hold ksplit * M * pad64(N) contiguous fp32 values")
    dst = out if ksplit == 1 else partial
    L.check(L.load().sda_sim_gemm_windows(_p(xm), x_pitch, _p(table), _p(starts), lo, row_elems, _p(dst), M, N, Np, K, ksplit,
                                          dt_code(xm.dtype), _st()), "sim_gemm_windows")
    if ksplit > 1:
        L.check(L.load().sda_reduce_slabs(_p(partial), _p(out), ksplit, M * Np, _st()), "reduce_slabs")
    return out


def window_sumsq(row_sq: torch.Tensor, starts: torch.Tensor, M: int, T: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[m] = sum of row_sq[starts[m] ... starts[m] + T) for m < M in a fixed order (sda_window_sumsq); the caller has checked
    the starts against the rows of row_sq."""
    _need_cuda(row_sq, starts, out)
    _need_values(row_sq, torch.float32, T, "window_sumsq: row_sq must be contiguous fp32 sums of at least T rows")
    _need_values(starts, torch.int32, M, "window_sumsq: starts must hold M contiguous int32 rows")
    out = torch.empty(M, dtype=torch.float32, device=row_sq.device) if out is None else out
    _need_values(out, torch.float32, M, "window_sumsq: out must hold M contiguous fp32 values")
    L.check(L.load().sda_window_sumsq(_p(row_sq), _p(starts), _p(out), M, T, _st()), "window_sumsq")
    return out


def matmul_nt_splitk(xm: torch.Tensor, wm: torch.Tensor, M: int, N: int, K: int, pitch: int) -> torch.Tensor:
    """S[i][j] = sum_k xm[i][k] * wm[j][k] (both K-contiguous rows with `pitch`), fp32 (M, pad64(N)) result.
    Runs conv_gemm in split-K mode + ordered slab reduction (loss.py:68)."""
    Np = L.pad_channels(N)
    tiles256, ksplit = splitk_plan(xm.dtype, M, N, K, pitch)
    partial = torch.empty((ksplit, M, Np), dtype=torch.float32, device=xm.device)
    out = partial[0] if ksplit == 1 else torch.empty((M, Np), dtype=torch.float32, device=xm.device)
    return matmul_nt_splitk_into(xm, wm, M, N, K, pitch, tiles256, ksplit, partial, out)


def bn_finalize(partial, ntiles, count, gamma, beta, running_mean, running_var, Cp, training, eps=1e-5, momentum=0.1,
                want_bwd_coef=False, batches_tracked=None):
    """Returns (mean, rstd, scale, shift[, bwd_coef]); bwd_coef = [4][Cp] (gamma, beta, mean, rstd), the table the
    data-gradient conv reads in its BatchNorm-backward statistics mode.  batches_tracked: the module's int64
    num_batches_tracked buffer, incremented by the same launch in training mode."""
    if batches_tracked is not None and (batches_tracked.dtype != torch.int64 or not batches_tracked.is_cuda):
        raise L.SdaError("bn_finalize: batches_tracked must be an int64 device tensor")
    dev = gamma.device
    buf = torch.empty((8 if want_bwd_coef else 4, Cp), dtype=torch.float32, device=dev)
    mean, rstd, scale, shift = buf[0], buf[1], buf[2], buf[3]
    coef = buf[4:] if want_bwd_coef else None
    L.check(L.load().sda_bn_finalize(_p(partial), ntiles, float(count), _p(gamma), _p(beta), eps, momentum,
                                     _p(running_mean), _p(running_var), _p(mean), _p(rstd), _p(scale), _p(shift),
                                     _p(coef), gamma.numel(), Cp, int(training), _p(batches_tracked), _st()), "bn_finalize")
    return (mean, rstd, scale, shift, coef) if want_bwd_coef else (mean, rstd, scale, shift)


def bn_gelu_forward(x, y, scale, shift, B, T):
    L.check(L.load().sda_bn_gelu_forward(_p(x), _p(y), _p(scale), _p(shift), B, T, x.shape[1], dt_code(x.dtype), _st()),
            "bn_gelu_forward")
    return y


def reduce_scratch(Cp, device):
    return torch.empty(L.load().sda_reduce_scratch_floats(Cp), dtype=torch.float32, device=device)


def bn_gelu_backward(dy, x, mean, rstd, gamma, beta, dx, B, T, scratch, count=None, allreduce=None, tile_stats=None, dy_is_dg=False):
    """Returns (dgamma, dbeta) summed over `count` rows (global sums when `allreduce` is given) and fills dx.
    tile_stats: per-tile (sum dg, sum dg*xhat) already produced by the conv that wrote dy (conv_gemm(bn_x=...));
    without it the sums take a pass of their own over dy and x."""
    if dy_is_dg and tile_stats is None:
        raise L.SdaError("bn_gelu_backward: dy_is_dg needs the statistics rows of the conv that wrote dg")
    Cp = x.shape[1]
    n = float(count if count is not None else B * T)
    sums = torch.empty((2, Cp), dtype=torch.float32, device=x.device)
    dgamma, dbeta = sums[0], sums[1]
    lib = L.load()
    if tile_stats is not None and allreduce is None:          # single process: sums + coefficients in one launch
        coef = torch.empty(6 * Cp, dtype=torch.float32, device=x.device)
        fn = lib.sda_bn_gelu_backward_from_stats_dg if dy_is_dg else lib.sda_bn_gelu_backward_from_stats
        L.check(fn(_p(tile_stats), tile_stats.shape[0], _p(dy), _p(x), _p(mean), _p(rstd),
                                                    _p(gamma), _p(beta), gamma.numel(), n,
                                                    _p(dgamma), _p(dbeta), _p(coef), _p(dx), B, T, Cp, dt_code(x.dtype), _st()),
                "bn_gelu_backward_from_stats")
        return dgamma, dbeta
    if tile_stats is not None:
        L.check(lib.sda_reduce_stats(_p(tile_stats), tile_stats.shape[0], _p(dbeta), _p(dgamma), Cp, _st()), "reduce_stats")
    else:
        L.check(lib.sda_bn_gelu_backward_reduce(_p(dy), _p(x), _p(mean), _p(rstd), _p(gamma), _p(beta), gamma.numel(), _p(scratch),
                                                _p(dgamma), _p(dbeta), B, T, Cp, dt_code(x.dtype), _st()), "bn_gelu_backward_reduce")
    if allreduce is not None:
        allreduce(sums)
    coef = torch.empty(6 * Cp, dtype=torch.float32, device=x.device)
    fn = lib.sda_bn_gelu_backward_apply_dg if dy_is_dg else lib.sda_bn_gelu_backward_apply
    L.check(fn(_p(dy), _p(x), _p(mean), _p(rstd), _p(gamma), _p(beta), gamma.numel(), _p(dgamma),
                                           _p(dbeta), n, _p(coef), _p(dx), B, T, Cp,
                                           dt_code(x.dtype), _st()), "bn_gelu_backward_apply")
    return dgamma, dbeta


def reduce_stats(stats: torch.Tensor) -> torch.Tensor:
    """Per-tile rows (n, 2, Cp) -> fp32 (2 * Cp,) = [column sums of slot 0 | of slot 1], summed in fixed order."""
    Cp = stats.shape[2]
    out = torch.empty(2 * Cp, dtype=torch.float32, device=stats.device)
    L.check(L.load().sda_reduce_stats(_p(stats), stats.shape[0], _p(out), _p(out[Cp:]), Cp, _st()), "reduce_stats")
    return out


def glu_forward(x, y, B, T):
    L.check(L.load().sda_glu_forward(_p(x), _p(y), B, T, y.shape[1], dt_code(x.dtype), _st()), "glu_forward")
    return y


def glu_backward(x, dy, dx, B, T):
    L.check(L.load().sda_glu_backward(_p(x), _p(dy), _p(dx), B, T, dy.shape[1], dt_code(x.dtype), _st()), "glu_backward")
    return dx


def gelu_backward(u, dz, du, B, T):
    L.check(L.load().sda_gelu_backward(_p(u), _p(dz), _p(du), B, T, u.shape[1], dt_code(u.dtype), _st()), "gelu_backward")
    return du


def glu_backward_colsum(x, dy, dx, B, T, scratch):
    """dx = GLU backward; returns the fp32 column sums of dx (2*Ch) = bias gradient of the conv that made x."""
    cs = torch.empty(2 * dy.shape[1], dtype=torch.float32, device=x.device)
    L.check(L.load().sda_glu_backward_colsum(_p(x), _p(dy), _p(dx), _p(cs), _p(scratch), B, T, dy.shape[1], dt_code(x.dtype), _st()),
            "glu_backward_colsum")
    return cs


def glu_backward_colsum_og(out, gate, dy, dx, B, T, scratch):
    """GLU backward after a fused forward (conv_gemm(flags=EPI_GLU)): `out` = value * sigmoid(gate) and `gate` instead of the
    [value | gate] buffer; same dx ([d value | d gate]) and column sums as glu_backward_colsum."""
    Ch = dy.shape[1]
    cs = torch.empty(2 * Ch, dtype=torch.float32, device=dy.device)
    L.check(L.load().sda_glu_backward_colsum_og(_p(out), _p(gate), _p(dy), _p(dx), _p(cs), _p(scratch), B, T, Ch,
                                                dt_code(dy.dtype), _st()), "glu_backward_colsum_og")
    return cs


def glu_backward_og(out, gate, dy, dx, B, T):
    """glu_backward_colsum_og's dx alone (a backward that wants no bias gradient): with no colsum the kernel leaves its per-row
    partial sums in a scratch buffer and launches no final reduction."""
    Ch = dy.shape[1]
    scratch = torch.empty(L.load().sda_reduce_scratch_rows(B, T) * 2 * Ch, dtype=torch.float32, device=dy.device)
    L.check(L.load().sda_glu_backward_colsum_og(_p(out), _p(gate), _p(dy), _p(dx), None, _p(scratch), B, T, Ch,
                                                dt_code(dy.dtype), _st()), "glu_backward_og")
    return dx


def gelu_backward_colsum(u, dz, du, B, T, scratch):
    cs = torch.empty(u.shape[1], dtype=torch.float32, device=u.device)
    L.check(L.load().sda_gelu_backward_colsum(_p(u), _p(dz), _p(du), _p(cs), _p(scratch), B, T, u.shape[1], dt_code(u.dtype), _st()),
            "gelu_backward_colsum")
    return cs


def colsum(x, B, T, scratch):
    out = torch.empty(x.shape[1], dtype=torch.float32, device=x.device)
    L.check(L.load().sda_colsum(_p(x), _p(out), _p(scratch), B, T, x.shape[1], dt_code(x.dtype), _st()), "colsum")
    return out


def wgrad_tile_m(Cout_p: int) -> int:
    """Row tile sda_wgrad_gemm picks for Cout_p output channels."""
    return L.load().sda_wgrad_tile_m(Cout_p)


def splitk_tile_co(Np: int) -> int:
    """Tile AS splitk_plan COUNTS IT, kept for bit-stability (it decides ksplit): at Np = 640 the kernel, conv_tile_co(Np, 1), takes 128."""
    return 160 if Np % 160 == 0 else (128 if Np % 128 == 0 else 64)


def bias_grad(cs, C, glu_half=0, glu_half_p=0):
    """Padded column sums -> bias gradient: a view when the unpadded vector is a prefix of the padded one (no GLU
    split, or GLU halves without padding between them); the un-packing kernel otherwise."""
    if glu_half == 0 or glu_half_p == glu_half:
        return cs[:C]
    return unpack_vector(cs, C, glu_half, glu_half_p)


def wgrad_args(dy, x, *, B, T, Cout_p, Cin_p, KS, dil, dy_pitch, x_pitch, rows_limit, dtype, flags=0, g=None, perm=None,
               seg_start=None, nseg=1, row0=L.ROW_PAD, sample_rows=None, dy_zero_row=0, out_e=None, out_pitch=0, co_valid=0,
               sub=None, rscale=None, acc_scale=None, out_scale=None) -> L.WgradArgs:
    """Every field of one sda_wgrad_gemm descriptor, from device addresses (ints or None), extents, pitches, flags and a dtype code.
    Slabs (the defaults): row-layout dy and x (row 0 is dy's all-zero row), one fp32 [KS][Cout_p][Cin_p] slab of g per sample segment.
    Typed: matrices of T rows (row0 = sample_rows = 0, dy_zero_row an all-zero row of dy), co_valid scaled rows of out_e, out_pitch apart."""
    return L.WgradArgs(dy, x, g, out_e, sub, rscale, out_scale, perm, seg_start, nseg, B, T, Cout_p, Cin_p, KS, dil, dy_pitch, x_pitch,
                       out_pitch, row0, L.rows_tp(T) if sample_rows is None else sample_rows, rows_limit, dy_zero_row, co_valid, dtype,
                       acc_scale, flags)                                                        # (the struct's field order: the cheap way)


def wgrad_gemm(dy, x, *, B, T, KS, dil, perm=None, seg_start=None, nseg=1, alg_dims=None, flat_rows=False):
    """fp32 slabs (nseg, KS, Cout_p, Cin_p) of dy^T x over the RL rows of the samples in each segment.
    alg_dims = (Cin, Cout) unpadded, only used to count algorithmic FLOPs when the timer is on.
    flat_rows: the caller guarantees that dy's pad rows (the 16 rows in front of every sample) are zero — true for every
    row-layout buffer the kernels of this library write (they only ever write valid rows of zero-initialised buffers) —
    so a segment of consecutive samples is contracted as one run of rows in whole K-chunks (SDA_WGRAD_FLAT_ROWS)."""
    g = torch.empty((nseg, KS, dy.shape[1], x.shape[1]), dtype=torch.float32, device=x.device)
    if nseg > 1 and seg_start is None:
        raise L.SdaError("wgrad_gemm: nseg > 1 needs seg_start")
    a = wgrad_args(_p(dy), _p(x), B=B, T=T, Cout_p=dy.shape[1], Cin_p=x.shape[1], KS=KS, dil=dil, dy_pitch=dy.shape[1],
                   x_pitch=x.shape[1], rows_limit=x.shape[0], dtype=dt_code(x.dtype), g=_p(g), perm=_p(perm), seg_start=_p(seg_start),
                   nseg=nseg, flags=L.WGRAD_FLAT_ROWS if flat_rows else 0)   # (with `perm`: every sample as whole chunks across its own padding)
    cin, cout = alg_dims if alg_dims is not None else (x.shape[1], dy.shape[1])
    _launch("wgrad_gemm", lambda: (("wgrad_gemm", str(x.dtype).replace("torch.", ""), wgrad_tile_m(dy.shape[1]), KS),
                                   2.0 * B * T * KS * cin * cout), L.load().sda_wgrad_gemm, a, "wgrad_gemm")
    return g


def reduce_slabs(slabs: torch.Tensor) -> torch.Tensor:
    n = slabs[0].numel()
    if slabs.shape[0] == 1:
        return slabs[0]
    out = torch.empty_like(slabs[0])
    L.check(L.load().sda_reduce_slabs(_p(slabs), _p(out), slabs.shape[0], n, _st()), "reduce_slabs")
    return out


def matmul_tn_typed(G, Ym, out, sub, rscale, *, M_rows, N_valid, K_cols, pitch, out_scale=None, acc_scale=None):
    """out[j][k] = out_scale * (acc_scale[j] * sum_i G[i][j] * Ym[i][k] - rscale[j] * sub[j][k])   (typed rows with `pitch`).
    G may be a column slice of a wider matrix: its row stride is the pitch read, its width the columns served."""
    if G.shape[0] < M_rows + 1:
        raise L.SdaError("matmul_tn_typed: G needs one trailing all-zero row")
    a = wgrad_args(_p(G), _p(Ym), B=1, T=M_rows, Cout_p=G.shape[1], Cin_p=K_cols, KS=1, dil=0, dy_pitch=G.stride(0), x_pitch=pitch,
                   rows_limit=M_rows, dtype=dt_code(Ym.dtype), row0=0, sample_rows=0, dy_zero_row=M_rows, out_e=_p(out),
                   out_pitch=pitch, co_valid=N_valid, sub=_p(sub), rscale=_p(rscale), acc_scale=_p(acc_scale), out_scale=_p(out_scale))
    L.check(L.load().sda_wgrad_gemm(C.byref(a), _st()), "wgrad_gemm(typed)")
    return out


def clip_dz(G, Yt, Zt, out, rscale, cscale, *, Bm, Bn, row_elems, out_scale=None):
    """out[j][k] = out_scale * (cscale[j] * sum_i G[i][j] Yt[i][k] - rscale[j] Zt[j][k]) — the loss's embedding gradient.
    One GPU's shapes (Bm <= 256, 16-bit) run on the streaming kernel (loss_gemm.hip); anything else on wgrad_gemm's typed output.
    G may be a column slice of a wider coefficient matrix (a rank's own speech columns of the all-gathered dY coefficients)."""
    if G.stride(1) != 1:
        raise L.SdaError("clip_dz: the coefficient matrix needs unit column stride")
    if L.load().sda_clip_dz_supported(Bm, Bn, row_elems, dt_code(Yt.dtype)):
        L.check(L.load().sda_clip_dz(_p(G), G.stride(0), _p(Yt), _p(Zt), _p(out), _p(cscale), _p(rscale), _p(out_scale), Bm, Bn, row_elems,
                                     dt_code(Yt.dtype), _st()), "clip_dz")
        return out
    return matmul_tn_typed(G, Yt, out, Zt, rscale, M_rows=Bm, N_valid=Bn, K_cols=row_elems, pitch=row_elems, out_scale=out_scale,
                           acc_scale=cscale)


def clip_neg_rows(N: int) -> int:
    """Rows the negatives' coefficient matrix is allocated and read with: N in whole 32-row K-steps (asked, not mirrored)."""
    return L.load().sda_clip_neg_rows(N)


def clip_dz_windows_span(row_elems: int) -> int:
    """Largest start - base_row one clip_dz_windows launch serves for table rows of `row_elems` elements (asked, not mirrored)."""
    return L.load().sda_clip_dz_windows_span(row_elems)


def _need_neg(who: str, N: int, Bn: int, **named):
    """fp32 device vectors of the negatives' tail: name=(tensor, count)."""
    if N < 1 or Bn < 1:
        raise L.SdaError(f"{who}: needs at least one negative and one brain column, got N={N}, Bn={Bn}")
    for name, (t, count) in named.items():
        _need_values(t, torch.float32, count, f"{who}: {name} must hold {count} contiguous fp32 values on the device")


def clip_neg_stats(S, wsq, zsq, temp, col_lse, Bn: int, N: int):
    """The negatives' logits m [Bn][N] (brain-major fp32) from their raw scores S [Bn][>= N] against the brain rows, and their
    share merged into col_lse IN PLACE: col_lse[j] <- logaddexp(col_lse[j], lse_n m[j][n]) (sda_clip_neg_stats)."""
    _need_cuda(S, wsq, zsq, temp, col_lse)
    if S.dtype != torch.float32 or S.dim() != 2 or S.stride(1) != 1 or S.shape[0] < Bn or S.shape[1] < N:
        raise L.SdaError(f"clip_neg_stats: S must be an fp32 (>= {Bn}, >= {N}) matrix with unit column stride")
    _need_neg("clip_neg_stats", N, Bn, wsq=(wsq, N), zsq=(zsq, Bn), temp=(temp, 1), col_lse=(col_lse, Bn))
    mlog = torch.empty((Bn, N), dtype=torch.float32, device=S.device)
    L.check(L.load().sda_clip_neg_stats(_p(S), S.stride(0), _p(wsq), _p(zsq), _p(temp), _p(mlog), _p(col_lse), Bn, N, _st()),
            "clip_neg_stats")
    return mlog


def clip_neg_grad(mlog, col_lse, wsq, zsq, temp, inv_norm, rscale, scalars, dtype):
    """(Gn, cscale_n) of the negatives' part of dZ (sda_clip_neg_grad): Gn [clip_neg_rows(N)][pad64(Bn)] of `dtype` with the rows
    from N on and the pad columns zero.  The negatives' shares are ADDED to rscale [Bn] and to scalars[1] (d loss / d temp), which
    clip_grad(_labels) has written before on the same stream."""
    _need_cuda(mlog, col_lse, wsq, zsq, temp, rscale, scalars)
    if dtype not in (torch.bfloat16, torch.float16):
        raise L.SdaError(f"clip_neg_grad: dtype {dtype}; the window path serves 16-bit storage only (bfloat16 or float16)")
    if mlog.dim() != 2:
        raise L.SdaError("clip_neg_grad: mlog must be the (Bn, N) logits of clip_neg_stats")
    Bn, N = mlog.shape
    _need_neg("clip_neg_grad", N, Bn, mlog=(mlog, Bn * N), col_lse=(col_lse, Bn), wsq=(wsq, N), zsq=(zsq, Bn), temp=(temp, 1),
              rscale=(rscale, Bn), scalars=(scalars, 2))
    dev = mlog.device
    Gn = torch.empty((clip_neg_rows(N), L.pad_channels(Bn)), dtype=dtype, device=dev)       # every element is written by the kernel
    cscale_n = torch.empty(Bn, dtype=torch.float32, device=dev)
    colpart = torch.empty(Bn, dtype=torch.float32, device=dev)
    L.check(L.load().sda_clip_neg_grad(_p(mlog), _p(col_lse), _p(wsq), _p(zsq), _p(temp), float(inv_norm), _p(Gn), Gn.shape[1],
                                       _p(cscale_n), _p(rscale), _p(colpart), _p(scalars), Bn, N, dt_code(dtype), _st()), "clip_neg_grad")
    return Gn, cscale_n


def clip_dz_windows(Gn, table, starts, lo: int, hi: int, out, cscale_n, *, N: int, Bn: int, T: int, out_scale=None):
    """out[j][ROW_PAD * Fp + k] += out_scale * cscale_n[j] * sum_{n < N} Gn[n][j] * table[starts[n] * Fp + k], k < T * Fp: the
    negatives' part of dZ on top of what clip_dz wrote into the row-layout buffer `out` (sda_clip_dz_windows).  `lo`, `hi`: the
    smallest and largest start, from the caller's host copy — a span that does not fit the kernel's 32-bit offset and a window
    past the table's end are refused here."""
    _need_cuda(Gn, table, starts, out, cscale_n, out_scale)
    _need_values(starts, torch.int32, N, "clip_dz_windows: starts must hold N contiguous int32 table rows")
    if table.dim() != 2 or not table.is_contiguous() or table.dtype not in (torch.bfloat16, torch.float16):
        raise L.SdaError("clip_dz_windows: the table must be a contiguous (rows, pad64(F)) matrix of bfloat16 or float16 (there is "
                         "no fp32 window path)")
    Fp = table.shape[1]
    K = T * Fp
    if Gn.dtype != table.dtype or out.dtype != table.dtype:
        raise L.SdaError("clip_dz_windows: Gn, the table and out must share one 16-bit dtype")
    if Gn.dim() != 2 or Gn.stride(1) != 1 or Gn.shape[0] < clip_neg_rows(N) or Gn.shape[1] < Bn:
        raise L.SdaError(f"clip_dz_windows: Gn must hold {clip_neg_rows(N)} rows (N in whole K-steps, zeros from row N on) of >= {Bn} columns")
    if not out.is_contiguous() or out.dim() != 2 or out.shape[1] != Fp or out.shape[0] < Bn * L.rows_tp(T):
        raise L.SdaError(f"clip_dz_windows: out must be a row-layout buffer of >= {Bn} samples of {L.rows_tp(T)} rows of {Fp} elements")
    _need_values(cscale_n, torch.float32, Bn, "clip_dz_windows: cscale_n must hold Bn contiguous fp32 values")
    if hi - lo > clip_dz_windows_span(Fp):
        raise L.SdaError(f"clip_dz_windows: the negatives' windows span table rows {lo} ... {hi}, more than the "
                         f"{clip_dz_windows_span(Fp)} rows (4 GB) one launch addresses")
    if lo < 0 or hi < lo or hi * Fp + K > table.numel():
        raise L.SdaError(f"clip_dz_windows: windows [{lo}, {hi}] x {K} elements leave the table of {table.numel()} elements")
    L.check(L.load().sda_clip_dz_windows(_p(Gn), Gn.stride(0), _p(table), _p(starts), lo, hi - lo, Fp, _p(out), L.rows_tp(T) * Fp,
                                         _p(cscale_n), _p(out_scale), N, Bn, K, dt_code(table.dtype), _st()), "clip_dz_windows")
    return out


def sa_gemm_tables(cos_t: torch.Tensor, sin_t: torch.Tensor):
    """Operand tables of SpatialAttention's two contractions, built from the (K2, C) cos/sin buffers:
    forward  a[o][c] = sum_m Re z[o][m] cos[m][c] + Im z[o][m] sin[m][c]  ->  rows c of [cos | sin] interleaved in m,
    backward dz[o][m] = sum_c da[o][c] (cos[m][c], sin[m][c])            ->  rows (2m, 2m+1), sensors padded to 64.
    The owner of the buffers (models.SpatialAttention) caches them and rebuilds when the buffers change."""
    K2, Cc = cos_t.shape
    both = torch.stack([cos_t, sin_t], dim=-1)                                    # (K2, C, 2)
    fwd = both.permute(1, 0, 2).reshape(Cc, 2 * K2).contiguous()
    Cq = (Cc + 63) // 64 * 64
    bwd = torch.zeros((2 * K2, Cq), dtype=torch.float32, device=cos_t.device)
    bwd[:, :Cc] = both.permute(0, 2, 1).reshape(2 * K2, Cc)
    return fwd, bwd


def sa_weights_forward(z, cos_t, sin_t, mask, D1p, Cp, dtype, fwd_table=None):
    """SpatialAttention weights (models.py:49-58) + dropout mask (81-84): W fp32 (D1, C) and the packed operand.
    The (D1 x 2K2) . (2K2 x C) contraction runs on the fp32 matrix path (conv_gemm, split-K matrix mode)."""
    D1, K2 = z.shape
    Cc = cos_t.shape[1]
    zr = torch.view_as_real(z).contiguous().view(D1, 2 * K2)
    W = torch.empty((D1, Cc), dtype=torch.float32, device=z.device)
    Wp = torch.empty((1, 1, D1p, Cp), dtype=dtype, device=z.device)
    if fwd_table is not None and (2 * K2) % 64 == 0:   # the matrix path contracts in whole 64-element slabs
        a = matmul_nt_splitk(zr, fwd_table, D1, Cc, 2 * K2, 2 * K2)                          # (D1, pad64(C)) fp32
        L.check(L.load().sda_sa_softmax_pack(_p(a), a.shape[1], _p(mask), _p(W), _p(Wp), D1, Cc, D1p, Cp, dt_code(dtype), _st()),
                "sa_softmax_pack")
        return W, Wp
    scratch = torch.empty(L.load().sda_sa_scratch_floats(D1, K2, Cc), dtype=torch.float32, device=z.device)
    L.check(L.load().sda_sa_weights_forward(_p(zr), _p(cos_t), _p(sin_t), _p(mask), _p(W), _p(Wp), _p(scratch), D1, K2, Cc, D1p, Cp,
                                            dt_code(dtype), _st()), "sa_weights_forward")
    return W, Wp


def sa_weights_backward(dWd, W, mask, cosT, sinT, K2, bwd_table=None):
    """dWd fp32 (rows >= D1, pitch dWd.shape[-1]) -> dz complex64 (D1, K2).  With `bwd_table` (sa_gemm_tables) the
    (D1 x C) . (C x 2K2) contraction runs on the fp32 matrix path; otherwise the stand-alone kernel is used."""
    D1, Cc = W.shape
    if bwd_table is not None and (2 * K2) % 64 == 0:
        bwd = bwd_table
        Cq = bwd.shape[1]
        da = torch.empty((D1, Cq), dtype=torch.float32, device=W.device)
        L.check(L.load().sda_sa_softmax_backward(_p(dWd), dWd.shape[-1], _p(W), _p(mask), _p(da), Cq, D1, Cc, _st()),
                "sa_softmax_backward")
        dz = matmul_nt_splitk(da, bwd, D1, 2 * K2, Cq, Cq)                              # (D1, 2*K2) = (re, im) interleaved
        return torch.view_as_complex(dz[:, : 2 * K2].reshape(D1, K2, 2))
    dz = torch.empty((D1, K2, 2), dtype=torch.float32, device=W.device)
    L.check(L.load().sda_sa_weights_backward(_p(dWd), _p(W), _p(mask), _p(cosT), _p(sinT), _p(dz), D1, K2, Cc, dWd.shape[-1],
                                             _st()), "sa_weights_backward")
    return torch.view_as_complex(dz)


def clip_logits_stats(S, ysq, zsq, temp, Bm, Bn, col0):
    dev = S.device
    logits = torch.empty((Bm, Bn), dtype=torch.float32, device=dev)
    # (row max, row sum, positive's logit) as the three rows of ONE buffer: under data parallelism that buffer is what the
    # all-gather of the row statistics sends — no stack / copy in front of the collective
    st3 = torch.empty((3, Bm), dtype=torch.float32, device=dev)
    row_max, row_sum, diag = st3[0], st3[1], st3[2]                    # (diag: every row is written, zero where the positive lives elsewhere)
    col_lse = torch.empty(Bn, dtype=torch.float32, device=dev)
    row_lse = torch.empty(Bm, dtype=torch.float32, device=dev)        # lse over THIS block of columns
    L.check(L.load().sda_clip_logits_stats(_p(S), S.shape[1], _p(ysq), _p(zsq), _p(temp), _p(logits), _p(row_max), _p(row_sum),
                                           _p(col_lse), _p(diag), _p(row_lse), Bm, Bn, col0, _st()), "clip_logits_stats")
    return logits, row_max, row_sum, col_lse, diag, row_lse


def clip_grad(logits, row_lse, col_lse, ysq, zsq, temp, inv_norm, col0, dtype):
    Bm, Bn = logits.shape
    dev = logits.device
    G = torch.empty((Bm + 1, L.pad_channels(Bn)), dtype=dtype, device=dev)      # + one zero row (wgrad_gemm's t >= T stand-in):
                                                                                 # it and the padding columns are written by the kernel
    rscale = torch.empty(Bn, dtype=torch.float32, device=dev)
    cscale = torch.empty(Bn, dtype=torch.float32, device=dev)
    colpart = torch.empty(2 * Bn, dtype=torch.float32, device=dev)
    scalars = torch.empty(2, dtype=torch.float32, device=dev)
    L.check(L.load().sda_clip_grad(_p(logits), _p(row_lse), _p(col_lse), _p(ysq), _p(zsq), _p(temp), float(inv_norm), col0,
                                   _p(G), G.shape[1], _p(rscale), _p(cscale), _p(colpart), _p(scalars), Bm, Bn, dt_code(dtype), _st()),
            "clip_grad")
    return G, rscale, cscale, scalars


def clip_grad_y(logits, row_lse, col_lse, zsq, zsq_all, col0, dtype, *, seg=None, seg_pitch=None, groups=1):
    """Coefficients of the speech-side gradient on one logits block (sda_clip_grad_y): Gy [Bn + 1][groups * seg_pitch] of `dtype`
    (column group g holds speech rows g * seg ... g * seg + seg - 1) and the per-row partials [ceil(Bn / 64)][Bm] fp32."""
    Bm, Bn = logits.shape
    seg = Bm if seg is None else seg
    seg_pitch = L.pad_channels(seg) if seg_pitch is None else seg_pitch
    dev = logits.device
    Gy = torch.empty((Bn + 1, groups * seg_pitch), dtype=dtype, device=dev)     # every element is written by the kernel
    part = torch.empty(((Bn + 63) // 64, Bm), dtype=torch.float32, device=dev)
    L.check(L.load().sda_clip_grad_y(_p(logits), _p(row_lse), _p(col_lse), _p(zsq), _p(zsq_all), zsq_all.numel(), col0, _p(Gy),
                                     Gy.shape[1], seg, seg_pitch, _p(part), Bm, Bn, dt_code(dtype), _st()), "clip_grad_y")
    return Gy, part


def clip_grad_y_finish(part, ysq, zsq_all, temp, inv_norm, row0, nrows):
    """part: [nparts][Bg] partials of every block in rank order -> (rscale_y, cscale_y) of speech rows [row0, row0 + nrows)."""
    nparts, Bg = part.shape
    rscale = torch.empty(nrows, dtype=torch.float32, device=part.device)
    cscale = torch.empty(nrows, dtype=torch.float32, device=part.device)
    L.check(L.load().sda_clip_grad_y_finish(_p(part), nparts, Bg, _p(ysq), _p(zsq_all), zsq_all.numel(), _p(temp), float(inv_norm),
                                            row0, nrows, _p(rscale), _p(cscale), _st()), "clip_grad_y_finish")
    return rscale, cscale


def clip_ranks(logits, diag, col0):
    Bm, Bn = logits.shape
    cnt = torch.empty(Bm, dtype=torch.int32, device=logits.device)
    L.check(L.load().sda_clip_ranks(_p(logits), _p(diag), _p(cnt), Bm, Bn, col0, _st()), "clip_ranks")
    return cnt


CLIP_DUPLICATES = {"positive": L.CLIP_DUP_POSITIVE, "mask": L.CLIP_DUP_MASK}


def clip_dup_code(duplicates: str) -> int:
    if duplicates not in CLIP_DUPLICATES:
        raise ValueError(f"duplicates must be one of {sorted(CLIP_DUPLICATES)}, got {duplicates!r}")
    return CLIP_DUPLICATES[duplicates]


def _need_labels(who: str, labels, n: int, *more):
    for name, t in (("labels", labels), *more):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() == n):
            raise L.SdaError(f"{who}: {name} must be a contiguous device int32 tensor of {n} values (one per global sample)")


def clip_label_counts(labels: torch.Tensor) -> torch.Tensor:
    """n_i = the number of samples of the global batch that carry sample i's speech label (itself included), int32 [Bg]."""
    _need_labels("clip_label_counts", labels, labels.numel() if isinstance(labels, torch.Tensor) else 0)
    counts = torch.empty_like(labels)
    L.check(L.load().sda_clip_label_counts(_p(labels), _p(counts), labels.numel(), _st()), "clip_label_counts")
    return counts


def clip_logits_stats_masked(S, ysq, zsq, temp, labels, Bm, Bn, col0):
    """clip_logits_stats with the repeats of a sample's own speech left out of both soft-max denominators (duplicates="mask")."""
    _need_labels("clip_logits_stats_masked", labels, Bm)
    dev = S.device
    logits = torch.empty((Bm, Bn), dtype=torch.float32, device=dev)
    st3 = torch.empty((3, Bm), dtype=torch.float32, device=dev)          # one buffer: what the all-gather of the row statistics sends
    row_max, row_sum, diag = st3[0], st3[1], st3[2]
    col_lse = torch.empty(Bn, dtype=torch.float32, device=dev)
    row_lse = torch.empty(Bm, dtype=torch.float32, device=dev)
    L.check(L.load().sda_clip_logits_stats_masked(_p(S), S.shape[1], _p(ysq), _p(zsq), _p(temp), _p(labels), _p(logits), _p(row_max),
                                                  _p(row_sum), _p(col_lse), _p(diag), _p(row_lse), Bm, Bn, col0, _st()),
            "clip_logits_stats_masked")
    return logits, row_max, row_sum, col_lse, diag, row_lse


def clip_grad_labels(logits, row_lse, col_lse, ysq, zsq, temp, labels, counts, duplicates, inv_norm, col0, dtype):
    """clip_grad with the labelled coefficient D (sda_clip_grad_labels): the same four results in the same layouts."""
    Bm, Bn = logits.shape
    mode = clip_dup_code(duplicates)
    _need_labels("clip_grad_labels", labels, Bm, ("counts", counts))
    dev = logits.device
    G = torch.empty((Bm + 1, L.pad_channels(Bn)), dtype=dtype, device=dev)      # zero row and pad columns written by the kernel
    rscale = torch.empty(Bn, dtype=torch.float32, device=dev)
    cscale = torch.empty(Bn, dtype=torch.float32, device=dev)
    colpart = torch.empty(2 * Bn, dtype=torch.float32, device=dev)
    scalars = torch.empty(2, dtype=torch.float32, device=dev)
    L.check(L.load().sda_clip_grad_labels(_p(logits), _p(row_lse), _p(col_lse), _p(ysq), _p(zsq), _p(temp), _p(labels), _p(counts), mode,
                                          float(inv_norm), col0, _p(G), G.shape[1], _p(rscale), _p(cscale), _p(colpart), _p(scalars),
                                          Bm, Bn, dt_code(dtype), _st()), "clip_grad_labels")
    return G, rscale, cscale, scalars


def clip_grad_y_labels(logits, row_lse, col_lse, zsq, zsq_all, labels, counts, duplicates, col0, dtype, *, seg=None, seg_pitch=None,
                       groups=1):
    """clip_grad_y with the labelled coefficient D (sda_clip_grad_y_labels): Gy and the partials in the same layouts."""
    Bm, Bn = logits.shape
    mode = clip_dup_code(duplicates)
    _need_labels("clip_grad_y_labels", labels, Bm, ("counts", counts))
    seg = Bm if seg is None else seg
    seg_pitch = L.pad_channels(seg) if seg_pitch is None else seg_pitch
    dev = logits.device
    Gy = torch.empty((Bn + 1, groups * seg_pitch), dtype=dtype, device=dev)     # every element is written by the kernel
    part = torch.empty(((Bn + 63) // 64, Bm), dtype=torch.float32, device=dev)
    L.check(L.load().sda_clip_grad_y_labels(_p(logits), _p(row_lse), _p(col_lse), _p(zsq), _p(zsq_all), zsq_all.numel(), _p(labels),
                                            _p(counts), mode, col0, _p(Gy), Gy.shape[1], seg, seg_pitch, _p(part), Bm, Bn,
                                            dt_code(dtype), _st()), "clip_grad_y_labels")
    return Gy, part


def clip_ranks_labels(logits, diag, labels, col0):
    """clip_ranks where the columns that carry the row's own speech label are never counted as beating its positive."""
    Bm, Bn = logits.shape
    _need_labels("clip_ranks_labels", labels, Bm)
    cnt = torch.empty(Bm, dtype=torch.int32, device=logits.device)
    L.check(L.load().sda_clip_ranks_labels(_p(logits), _p(diag), _p(labels), _p(cnt), Bm, Bn, col0, _st()), "clip_ranks_labels")
    return cnt


def _sigmoid_args(who: str, labels, duplicates, Bm: int, Bn: int, col0: int, *tensors):
    """What the three sigmoid entry points check before anything is launched -> the C `mode`."""
    mode = clip_dup_code(duplicates)
    if Bm < 1 or Bn < 1 or col0 < 0 or col0 + Bn > Bm:
        raise L.SdaError(f"{who}: need Bm, Bn >= 1 and 0 <= col0, col0 + Bn <= Bm, got Bm={Bm} Bn={Bn} col0={col0}")
    if labels is not None:
        _need_labels(who, labels, Bm)
    _need_cuda(*tensors)
    return mode


def sigmoid_pairs(S, ysq, zsq, temp, bias, Bm, Bn, col0, dtype, labels=None, duplicates="positive"):
    """One pass over a block of the pairwise sigmoid loss (sda_sigmoid_pairs): a = the scaled cosines fp32 (Bm, Bn), diag as
    clip_logits_stats leaves it, G (Bm + 1, pad64(Bn)) of `dtype` and the per-column partials (ceil(Bm / 64), Bn, 3)."""
    mode = _sigmoid_args("sigmoid_pairs", labels, duplicates, Bm, Bn, col0, S, ysq, zsq, temp, bias)
    dev = S.device
    a = torch.empty((Bm, Bn), dtype=torch.float32, device=dev)
    diag = torch.empty(Bm, dtype=torch.float32, device=dev)
    G = torch.empty((Bm + 1, L.pad_channels(Bn)), dtype=dtype, device=dev)      # zero row and pad columns written by the kernel
    part = torch.empty(((Bm + 63) // 64, Bn, 3), dtype=torch.float32, device=dev)
    L.check(L.load().sda_sigmoid_pairs(_p(S), S.shape[1], _p(ysq), _p(zsq), _p(temp), _p(bias), _p(labels), mode, col0, _p(a), _p(diag),
                                       _p(G), G.shape[1], _p(part), Bm, Bn, dt_code(dtype), _st()), "sigmoid_pairs")
    return a, diag, G, part


def sigmoid_finish(part, ysq, zsq, temp, inv_norm):
    """The partials of sigmoid_pairs -> (rscale, cscale) of clip_dz's contract and scalars[3] = this block's shares of
    (loss, d loss / d temp, d loss / d bias)."""
    _need_cuda(part, ysq, zsq, temp)
    nparts, Bn, _ = part.shape
    Bm = ysq.numel()
    rscale = torch.empty(Bn, dtype=torch.float32, device=part.device)
    cscale = torch.empty(Bn, dtype=torch.float32, device=part.device)
    scalars = torch.empty(3, dtype=torch.float32, device=part.device)
    L.check(L.load().sda_sigmoid_finish(_p(part), nparts, _p(ysq), _p(zsq), _p(temp), float(inv_norm), _p(rscale), _p(cscale),
                                        _p(scalars), Bm, Bn, _st()), "sigmoid_finish")
    return rscale, cscale, scalars


def sigmoid_grad_y(a, bias, zsq, zsq_all, col0, dtype, labels=None, duplicates="positive", *, seg=None, seg_pitch=None, groups=1):
    """clip_grad_y's twin for the sigmoid loss (sda_sigmoid_grad_y): Gy and the per-row partials in the same layouts, D
    recomputed from a, bias and the labels."""
    Bm, Bn = a.shape
    mode = _sigmoid_args("sigmoid_grad_y", labels, duplicates, Bm, Bn, col0, a, bias, zsq, zsq_all)
    seg = Bm if seg is None else seg
    seg_pitch = L.pad_channels(seg) if seg_pitch is None else seg_pitch
    dev = a.device
    Gy = torch.empty((Bn + 1, groups * seg_pitch), dtype=dtype, device=dev)     # every element is written by the kernel
    part = torch.empty(((Bn + 63) // 64, Bm), dtype=torch.float32, device=dev)
    L.check(L.load().sda_sigmoid_grad_y(_p(a), _p(bias), _p(zsq), _p(zsq_all), zsq_all.numel(), _p(labels), mode, col0, _p(Gy),
                                        Gy.shape[1], seg, seg_pitch, _p(part), Bm, Bn, dt_code(dtype), _st()), "sigmoid_grad_y")
    return Gy, part


def retrieval_scores_floats(n: int, M: int, chunk_cols: int) -> int:
    """Floats of the chunk-major score matrix sda_retrieval_select reads for n query rows against M candidates."""
    r = L.load().sda_retrieval_scores_floats(n, M, chunk_cols)
    if r < 0:
        L.check(-1, "retrieval_scores_floats")
    return r


def _need_scores(who: str, S, qsq, csq, n: int, M: int, chunk_cols: int):
    """The operands retrieval_select and retrieval_class_reduce share: the chunk-major scores and the two sides' norms."""
    _need_values(S, torch.float32, retrieval_scores_floats(n, M, chunk_cols),
                 "{}: S must be a contiguous fp32 buffer of retrieval_scores_floats(n, M, chunk_cols) floats", who)
    for t, cnt, name in ((qsq, n, "qsq"), (csq, M, "csq")):
        _need_values(t, torch.float32, cnt, "{}: {} must hold {} contiguous fp32 values", who, name, cnt)


def retrieval_select(S, qsq, csq, n: int, M: int, k: int, chunk_cols: Optional[int] = None, labels=None, indices=None, scores=None,
                     ranks=None):
    """Top-k of n query rows over the raw dot products S (chunk-major, see sd_amd.h; chunk_cols None = one [n][pad64(M)] matrix)
    with the squared norms qsq [n], csq [M] -> (indices (n, k) int64, scores (n, k) fp32, ranks (n,) int32 or None).  `labels`:
    n int64 candidate indices on the device.  The three outputs may be handed in (contiguous row blocks of larger results)."""
    _need_cuda(S, qsq, csq, labels)
    chunk_cols = L.pad_channels(M) if chunk_cols is None else chunk_cols
    _need_scores("retrieval_select", S, qsq, csq, n, M, chunk_cols)
    _need_values(labels, torch.int64, n, "retrieval_select: labels must hold n contiguous int64 indices")
    dev = S.device
    indices = torch.empty((n, k), dtype=torch.int64, device=dev) if indices is None else indices
    scores = torch.empty((n, k), dtype=torch.float32, device=dev) if scores is None else scores
    if labels is not None and ranks is None:
        ranks = torch.empty(n, dtype=torch.int32, device=dev)
    for t, dt, cnt in ((indices, torch.int64, n * k), (scores, torch.float32, n * k), (ranks, torch.int32, n)):
        _need_values(t, dt, cnt, "retrieval_select: an output buffer has the wrong dtype, size or layout")
    L.check(L.load().sda_retrieval_select(_p(S), _p(qsq), _p(csq), _p(labels), _p(indices), _p(scores),
                                          _p(ranks) if labels is not None else None, n, M, k, chunk_cols, _st()), "retrieval_select")
    return indices, scores, (ranks if labels is not None else None)


CLASS_MODES = {"sum": 0, "mean": 1, "max": 2}


def retrieval_class_reduce(S, qsq, csq, order, offsets, n: int, M: int, C: int, scale: float, mode: str = "sum",
                           chunk_cols: Optional[int] = None, out=None, row_lse=None):
    """Class values of n query rows over the raw dot products S (chunk-major, as retrieval_select reads them): the M candidates
    fall into C classes given as the CSR index order [M] / offsets [C + 1] (device int32) -> (out (n, pad64(C)) fp32 of which
    columns [0, C) are written: log-sum-exp ("sum"), that minus log n_c ("mean") or the maximum ("max") of scale * cosine over
    the class, minus the row's log-sum-exp; row_lse (n,) fp32).  See sd_amd.h.  `out` (rows of a larger matrix, any pitch >= C)
    and `row_lse` may be handed in."""
    _need_cuda(S, qsq, csq, order, offsets, out, row_lse)
    if mode not in CLASS_MODES:
        raise L.SdaError(f"retrieval_class_reduce: mode {mode!r}; one of {sorted(CLASS_MODES)}")
    chunk_cols = L.pad_channels(M) if chunk_cols is None else chunk_cols
    _need_scores("retrieval_class_reduce", S, qsq, csq, n, M, chunk_cols)
    for t, cnt, name in ((order, M, "order"), (offsets, C + 1, "offsets")):
        _need_values(t, torch.int32, cnt, "retrieval_class_reduce: {} must hold {} contiguous int32 values", name, cnt)
    dev = S.device
    out = torch.empty((n, L.pad_channels(C)), dtype=torch.float32, device=dev) if out is None else out
    row_lse = torch.empty(n, dtype=torch.float32, device=dev) if row_lse is None else row_lse
    _need_fp32_rows(out, n, C, "retrieval_class_reduce: out must be n fp32 rows of at least C contiguous columns")
    _need_values(row_lse, torch.float32, n, "retrieval_class_reduce: row_lse must hold n contiguous fp32 values")
    L.check(L.load().sda_retrieval_class_reduce(_p(S), _p(qsq), _p(csq), _p(order), _p(offsets), _p(out), _p(row_lse),
                                                out.stride(0), n, M, C, chunk_cols, float(scale), CLASS_MODES[mode], _st()),
            "retrieval_class_reduce")
    return out, row_lse


def retrieval_pool_rows(V, rows, group_offsets, N: int, G: int, C: int, out=None):
    """out[g][c] = log mean exp of V[r][c] over the rows r of group g (rows [N] / group_offsets [G + 1], device int32: the row
    list sorted by group, see sd_amd.h) for c < C; V (N, >= C) fp32 rows -> out (G, pad64(C)) fp32, columns >= C not written."""
    _need_cuda(V, rows, group_offsets, out)
    out = torch.empty((G, L.pad_channels(C)), dtype=torch.float32, device=V.device) if out is None else out
    for t, cnt in ((V, N), (out, G)):
        _need_fp32_rows(t, cnt, C, "retrieval_pool_rows: V and out must be fp32 rows of at least C contiguous columns")
    for t, cnt, name in ((rows, N, "rows"), (group_offsets, G + 1, "group_offsets")):
        _need_values(t, torch.int32, cnt, "retrieval_pool_rows: {} must hold {} contiguous int32 values", name, cnt)
    L.check(L.load().sda_retrieval_pool_rows(_p(V), V.stride(0), _p(rows), _p(group_offsets), _p(out), out.stride(0), N, G, C, _st()),
            "retrieval_pool_rows")
    return out


# ---------------------------------------------------------------------------------------------------------------
# wav2vec 2.0 embedder stages (csrc/w2v2.hip) and the raw GEMM form of conv_gemm they share
# ---------------------------------------------------------------------------------------------------------------
def gemm_view(x_ptr: int, w_ptr: int, y_ptr: int, *, rows: int, K: int, Cout_p: int, x_pitch: int, w_pitch: int, x_row0: int,
              x_rows_limit: int, dtype, bias=None, res_ptr: Optional[int] = None, gelu: bool = False,
              w_rows_limit: Optional[int] = None, batch: int = 1, sample_rows: Optional[int] = None, widx=None):
    """y[x_row0 + r][0:Cout_p] = sum_k x[x_row0 + r][k] * w[co][k] (+ bias)(+ res)(GELU) for r < rows, on raw device
    addresses: conv_gemm with kernel size 1 in matrix mode.  Row r of x starts at x_ptr + (x_row0 + r) * x_pitch elements
    and is K elements long, so x_pitch < K gives overlapping rows (an im2col view of a strided Conv1d); w row co starts at
    w_ptr + co * w_pitch.  y rows have Cout_p elements.  The caller guarantees every address touched is allocated."""
    # `batch` independent problems of `rows` rows each, `sample_rows` view rows apart (x and y alike); widx[b] picks the
    # b-th problem's weight matrix out of w [nW][Cout_p][w_pitch]
    a = conv_args(x_ptr, w_ptr, y_ptr, B=batch, T=rows, Cin_p=K, Cout_p=Cout_p, KS=1, dil=0, x_pitch=x_pitch, w_pitch=w_pitch,
                  x_rows_limit=x_rows_limit, dtype=dt_code(dtype), flags=L.EPI_GELU if gelu else 0, bias=_p(bias), res=res_ptr,
                  widx=_p(widx), x_row0=x_row0, x_sample_rows=sample_rows, w_rows_limit=w_rows_limit)
    L.check(L.load().sda_conv_gemm(C.byref(a), _st()), "conv_gemm(view)")


def w2v_conv0(wave, w, bias, gamma, beta, y, T, C, K, stride, eps=1e-5):
    L.check(L.load().sda_w2v_conv0(_p(wave), wave.numel(), _p(w), _p(bias), _p(gamma), _p(beta), _p(y), T, C, y.shape[1], K, stride,
                                   eps, dt_code(y.dtype), _st()), "w2v_conv0")
    return y


INT_MAX = 2 ** 31 - 1


def _need_conv0_frames(who: str, wave, T: int, K: int, stride: int):
    """The frame count and the waveform of a layer-0 launch, or SdaError: T travels as a C int."""
    if not 1 <= T <= INT_MAX - L.ROW_PAD:
        raise L.SdaError(f"{who}: {T} frames; 1 <= frames <= {INT_MAX - L.ROW_PAD} (a C int holds the row index)")
    _need_values(wave, torch.float32, (T - 1) * stride + K, "{}: wave is {} contiguous fp32 samples on the device", who,
                 (T - 1) * stride + K)


def w2v_conv0_stats_floats(T: int, C: int) -> int:
    """Floats of scratch `w2v_conv0_stats` needs for T frames of C channels: shift[C], mean[C], rstd[C], then the workgroups' partials."""
    if not 1 <= T <= INT_MAX - L.ROW_PAD or C < 1:
        raise L.SdaError(f"w2v_conv0_stats_floats: {T} frames of {C} channels; 1 <= frames <= {INT_MAX - L.ROW_PAD}, channels >= 1")
    return int(L.load().sda_w2v_conv0_stats_floats(T, C))


def w2v_conv0_stats(wave, w, bias, scratch, T, C, K, stride, eps=1e-5):
    """Per-channel statistics of x = Conv1d(1 -> C, K, stride)(wave) over all T frames, left in scratch[:3C]: shift = x at
    frame 0, the mean of x - shift, rsqrt(biased variance + eps) (`sda_w2v_conv0_stats`); returns that (3, C) view.  scratch: fp32, at least
    w2v_conv0_stats_floats(T, C) values, the caller's (one per stream in flight)."""
    _need_conv0_frames("w2v_conv0_stats", wave, T, K, stride)
    _need_values(w, torch.float32, C * K, "w2v_conv0_stats: w is fp32 [{}][{}] on the device", C, K)
    _need_values(bias, torch.float32, C, "w2v_conv0_stats: bias is {} fp32 values on the device", C)
    _need_values(scratch, torch.float32, w2v_conv0_stats_floats(T, C), "w2v_conv0_stats: scratch holds w2v_conv0_stats_floats({}, {}) fp32 "
                 "values on the device", T, C)
    L.check(L.load().sda_w2v_conv0_stats(_p(wave), wave.numel(), _p(w), _p(bias), _p(scratch), scratch.numel(), T, C, K, stride, eps,
                                         _st()), "w2v_conv0_stats")
    return scratch[:3 * C].view(3, C)


def w2v_conv0_groupnorm(wave, w, bias, gamma, beta, stats, y, T, C, K, stride):
    """y[ROW_PAD + t] = GELU(gamma ((conv(wave)[t] - shift) - mean) rstd + beta) with stats = the (3, C) of w2v_conv0_stats;
    pad channels of those rows are written as zero (`sda_w2v_conv0_groupnorm`)."""
    _need_conv0_frames("w2v_conv0_groupnorm", wave, T, K, stride)
    _need_values(w, torch.float32, C * K, "w2v_conv0_groupnorm: w is fp32 [{}][{}] on the device", C, K)
    for name, t in (("bias", bias), ("gamma", gamma), ("beta", beta)):
        _need_values(t, torch.float32, C, "w2v_conv0_groupnorm: {} is {} fp32 values on the device", name, C)
    _need_values(stats, torch.float32, 3 * C, "w2v_conv0_groupnorm: stats is fp32 [3][{}] on the device", C)
    if not y.is_cuda or y.dim() != 2 or not y.is_contiguous() or y.shape[0] < L.ROW_PAD + T or C > y.shape[1]:
        raise L.SdaError(f"w2v_conv0_groupnorm: y is a row-layout device buffer of at least {L.ROW_PAD + T} rows and {C} channels")
    L.check(L.load().sda_w2v_conv0_groupnorm(_p(wave), wave.numel(), _p(w), _p(bias), _p(gamma), _p(beta), _p(stats), _p(y), T, C,
                                             y.shape[1], K, stride, dt_code(y.dtype), _st()), "w2v_conv0_groupnorm")
    return y


def layernorm_rows(x, y, gamma, beta, T, C, eps=1e-5, gelu=False):
    L.check(L.load().sda_layernorm_rows(_p(x), _p(y), _p(gamma), _p(beta), T, C, x.shape[1], eps, int(gelu), dt_code(x.dtype), _st()),
            "layernorm_rows")
    return y


def w2v_group_split(h, xg, T, gw, G, lead):
    L.check(L.load().sda_w2v_group_split(_p(h), _p(xg), T, h.shape[1], gw, xg.shape[2], G, xg.shape[1], lead, dt_code(h.dtype), _st()),
            "w2v_group_split")


def w2v_group_merge_add(h, yg, out, T, gw, G, bias=None, gelu=False):
    L.check(L.load().sda_w2v_group_merge_add(_p(h), _p(yg), _p(out), T, h.shape[1], gw, yg.shape[2], G, yg.shape[1],
                                             _p(bias), int(gelu), dt_code(h.dtype), _st()), "w2v_group_merge_add")
    return out


def w2v_attention(q_ptr, k_ptr, vt, out, T, heads, head_dim, qk_pitch, scale):
    L.check(L.load().sda_w2v_attention(q_ptr, k_ptr, _p(vt), _p(out), T, heads, head_dim, qk_pitch, vt.shape[1], out.shape[1],
                                       scale, dt_code(out.dtype), _st()), "w2v_attention")
    return out


def w2v_mean4(a, b, c, d, T, Cc):
    out = torch.empty((T, Cc), dtype=torch.float32, device=a.device)
    L.check(L.load().sda_w2v_mean4(_p(a), _p(b), _p(c), _p(d), _p(out), T, Cc, a.shape[1], dt_code(a.dtype), _st()), "w2v_mean4")
    return out


def linear_rows_ksplit(T: int, Cout_p: int, Cin_p: int, dtype) -> int:
    """K slices linear_rows cuts its contraction into (256 workgroups at the most); < 2: the direct path, no scratch."""
    return min(Cin_p // k_slab(dtype), max(1, 256 // (n_t_tiles(T) * (Cout_p // conv_tile_co(Cout_p, 1)))))


def linear_rows(x, w, y, T, *, bias=None, res=None, gelu=False, scratch=None):
    """y = f(x W^T + bias) + res on ONE row-layout sample of T frames (w packed (1, 1, Cout_p, Cin_p)).  Few frames make
    few output tiles (a 1024-wide layer at T = 299 is 24 workgroups): then the contraction is split over workgroups
    (sda_conv_gemm's split-K slabs) and a small epilogue kernel sums the slabs and applies bias / GELU / residual."""
    Cout_p, Cin_p = w.shape[-2], w.shape[-1]
    ksplit = linear_rows_ksplit(T, Cout_p, Cin_p, x.dtype)
    if ksplit < 2:
        return conv_gemm(x, w, y, B=1, T=T, KS=1, dil=0, bias=bias, res=res, gelu=gelu)
    need = ksplit * T * Cout_p
    if scratch is None or scratch.numel() < need:
        scratch = torch.empty(need, dtype=torch.float32, device=x.device)
    a = conv_args(_p(x), _p(w), None, B=1, T=T, Cin_p=Cin_p, Cout_p=Cout_p, KS=1, dil=0, x_pitch=x.shape[1], w_pitch=Cin_p,
                  x_rows_limit=x.shape[0], dtype=dt_code(x.dtype), ksplit=ksplit, partial=_p(scratch))
    L.check(L.load().sda_conv_gemm(C.byref(a), _st()), "conv_gemm(split-K)")
    L.check(L.load().sda_splitk_epilogue(_p(scratch), ksplit, _p(bias), _p(res), _p(y), T, Cout_p, int(gelu), dt_code(x.dtype), _st()),
            "splitk_epilogue")
    return y


def mel_power(spec: torch.Tensor, fb: torch.Tensor, log_eps: Optional[float] = None) -> torch.Tensor:
    """`sda_mel_power_f32` (csrc/mel_power.hip): spec (..., frames, n_freqs, 2) contiguous fp32, real and imaginary parts
    interleaved as the STFT window GEMM leaves them, fb (n_freqs, n_mels) contiguous fp32 -> fp32 (..., n_mels, frames):
    out[..., j, m] = sum_b (re^2 + im^2)[..., m, b] fb[b, j], or logf(log_eps + that) when log_eps is given (>= 0)."""
    _need_cuda(spec, fb)
    if spec.dtype != torch.float32 or fb.dtype != torch.float32 or not spec.is_contiguous() or not fb.is_contiguous():
        raise L.SdaError("mel_power: contiguous fp32 tensors")
    if spec.dim() < 3 or spec.shape[-1] != 2 or fb.dim() != 2 or fb.shape[0] != spec.shape[-2]:
        raise L.SdaError(f"mel_power: spec (..., frames, n_freqs, 2) and fb (n_freqs, n_mels), got {tuple(spec.shape)} and {tuple(fb.shape)}")
    if log_eps is not None and not log_eps >= 0:
        raise L.SdaError("mel_power: log_eps must be None (no log) or >= 0")
    frames, n_freqs = spec.shape[-3], spec.shape[-2]
    n_mels = fb.shape[1]
    lead = tuple(spec.shape[:-3])
    rows = int(np.prod(lead, dtype=np.int64)) if lead else 1
    out = torch.empty(lead + (n_mels, frames), dtype=torch.float32, device=spec.device)
    with torch.cuda.device(spec.device):
        L.check(L.load().sda_mel_power_f32(_p(spec), frames * n_freqs * 2, n_freqs * 2, rows, frames, n_freqs, _p(fb), n_mels,
                                           -1.0 if log_eps is None else float(log_eps), _p(out), n_mels * frames, frames, _st()),
                "mel_power")
    return out


STFT_FFT_SIZES = (32, 64, 128, 256, 512, 1024, 2048)     # the n_fft `sda_stft_fft_f32` is instantiated for


def stft_fft_frames_per_workgroup(n_fft: int) -> int:
    """Frames one workgroup of `sda_stft_fft_f32` owns (csrc/stft_fft.hip: SF_SAMPLES / n_fft, at most SF_MAX_FRAMES)."""
    return min(4096 // int(n_fft), 32)


def stft_fft(rows_padded: torch.Tensor, window: torch.Tensor, twiddle: torch.Tensor, frames: int, hop: int, n_fft: int) -> torch.Tensor:
    """`sda_stft_fft_f32` (csrc/stft_fft.hip): rows_padded (rows, >= (frames - 1) hop + n_fft) contiguous fp32, window (n_fft,)
    and twiddle (n_fft / 2, 2) = (cos, -sin)(2 pi j / n_fft) contiguous fp32 -> fp32 (rows, frames, n_fft / 2 + 1, 2):
    the one-sided spectrum of window * frame, frames `hop` samples apart, in the layout `mel_power` reads."""
    _need_cuda(rows_padded, window, twiddle)
    n_fft, hop, frames = int(n_fft), int(hop), int(frames)
    if n_fft not in STFT_FFT_SIZES:
        raise L.SdaError(f"stft_fft: n_fft = {n_fft} is not one of {STFT_FFT_SIZES} (no fallback)")
    for t in (rows_padded, window, twiddle):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise L.SdaError("stft_fft: contiguous fp32 tensors")
    if rows_padded.dim() != 2 or tuple(window.shape) != (n_fft,) or tuple(twiddle.shape) != (n_fft // 2, 2):
        raise L.SdaError(f"stft_fft: rows (rows, L), window (n_fft,) and twiddle (n_fft / 2, 2), got {tuple(rows_padded.shape)}, "
                         f"{tuple(window.shape)} and {tuple(twiddle.shape)}")
    rows, n_freqs = rows_padded.shape[0], n_fft // 2 + 1
    out = torch.empty((rows, frames, n_freqs, 2), dtype=torch.float32, device=rows_padded.device)
    with torch.cuda.device(rows_padded.device):
        L.check(L.load().sda_stft_fft_f32(_p(rows_padded), rows_padded.shape[1], rows, frames, hop, n_fft, _p(window), _p(twiddle),
                                          _p(out), frames * n_freqs * 2, n_freqs * 2, _st()), "stft_fft")
    return out


# ---- lag products of the time-lagged ridge baseline (csrc/lagged_cov.hip) ----
def lagged_cov_slices(rows: int, n_lags: int, Ap: int, Bp: int) -> int:
    """Row slices (= slabs) `lagged_cov` writes for this shape: `sda_lagged_cov_slices`, a function of the four numbers alone."""
    n = int(L.load().sda_lagged_cov_slices(int(rows), int(n_lags), int(Ap), int(Bp)))
    if n < 0:
        L.check(-1, "lagged_cov_slices")
    return n


def lagged_cov(a: torch.Tensor, b: torch.Tensor, n_lags: int, H: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`sda_lagged_cov_f32`: a (rows, Ap) and b (rows, Bp) fp32 lag-layout buffers (rows of channels, pad channels zero, H >=
    n_lags - 1 zero rows behind every sample; a row stride wider than the width is taken as the pitch) -> the slabs
    (slices, n_lags, Ap, Bp) fp32, slab[s][d][i][j] = sum over the rows r of slice s of a[r + d][i] b[r][j].  Every element is
    written; the caller sums the slabs in fixed order (`reduce_slabs`, or in double).  `out`: a contiguous fp32 tensor to write
    them into instead of a new one."""
    _need_cuda(a, b, out)
    for t in (a, b):
        if t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1 or t.stride(0) < t.shape[1]:
            raise L.SdaError("lagged_cov: a and b are fp32 (rows, channels) device tensors with unit-stride channels")
    if a.shape[0] != b.shape[0]:
        raise L.SdaError(f"lagged_cov: a has {a.shape[0]} rows, b {b.shape[0]}")
    rows, Ap, Bp, n_lags = a.shape[0], a.shape[1], b.shape[1], int(n_lags)
    shape = (lagged_cov_slices(rows, n_lags, Ap, Bp), n_lags, Ap, Bp)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=a.device)
    elif out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != shape:
        raise L.SdaError(f"lagged_cov: out must be a contiguous fp32 tensor of shape {shape}")
    with torch.cuda.device(a.device):
        L.check(L.load().sda_lagged_cov_f32(_p(a), a.stride(0), _p(b), b.stride(0), rows, n_lags, int(H), Ap, Bp, _p(out), _st()),
                "lagged_cov")
    return out


# ---- gradient guard (csrc/grad_guard.hip, csrc/param_ops.hip): three launches over Adam's descriptor table, no read-back ----
def grad_guard_parts(n: int, max_n: int) -> int:
    """Doubles `grad_sumsq_multi` writes for n tensors of at most max_n elements: 2 n gx, gx = min(ceil(max_n / 1024), 256)."""
    parts = int(L.load().sda_grad_guard_parts(int(n), int(max_n)))
    if parts < 0:
        L.check(-1, "grad_guard_parts")
    return parts


def _need_guard_state(state: torch.Tensor, who: str):
    _need_values(state, torch.float64, L.GUARD_STATE, "{}: state is {} contiguous device doubles", who, L.GUARD_STATE)


def grad_sumsq_multi(table: torch.Tensor, n: int, max_n: int, partials: torch.Tensor) -> torch.Tensor:
    """`sda_grad_sumsq_multi`: partials[t][b] = (sum of g^2 over the finite elements, count of the non-finite ones) of the slice
    of tensor t that Adam's workgroup b updates; table: the uploaded sda_adam_desc array of n entries.  Every slot is written."""
    _need_cuda(table)
    _need_values(partials, torch.float64, grad_guard_parts(n, max_n), "grad_sumsq_multi: partials holds {} contiguous device doubles",
                 grad_guard_parts(n, max_n))
    L.check(L.load().sda_grad_sumsq_multi(_p(table), int(n), int(max_n), _p(partials), _st()), "grad_sumsq_multi")
    return partials


def grad_guard_finish(partials: torch.Tensor, n: int, gx: int, state: torch.Tensor, max_norm: float, beta1: float, beta2: float,
                      growth_interval: int, max_scale: float, dynamic: bool) -> torch.Tensor:
    """`sda_grad_guard_finish`: the step's decision from the n x gx partial slots into `state` (lib.GUARD_* slots), on the device."""
    _need_values(partials, torch.float64, 2 * int(n) * int(gx), "grad_guard_finish: partials holds {} contiguous device doubles",
                 2 * int(n) * int(gx))
    _need_guard_state(state, "grad_guard_finish")
    L.check(L.load().sda_grad_guard_finish(_p(partials), int(n), int(gx), _p(state), float(max_norm), float(beta1), float(beta2),
                                           int(growth_interval), float(max_scale), int(bool(dynamic)), _st()), "grad_guard_finish")
    return state


def adam_multi_guarded(table: torch.Tensor, n: int, max_n: int, lr: float, beta1: float, beta2: float, eps: float,
                       state: torch.Tensor) -> None:
    """`sda_adam_multi_guarded`: Adam over the table's tensors on grad * (float)state[COEF], or nothing when state[SKIP] is set."""
    _need_cuda(table)
    _need_guard_state(state, "adam_multi_guarded")
    L.check(L.load().sda_adam_multi_guarded(_p(table), int(n), int(max_n), float(lr), float(beta1), float(beta2), float(eps),
                                            _p(state), _st()), "adam_multi_guarded")
