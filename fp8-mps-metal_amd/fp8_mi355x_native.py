"""
FP8 ops on MI355X (e4m3fn; float8_e5m2 operands and casts, OCP semantics, see the end of this note): the op layer between the monkey-patch
(fp8_mps_patch.py) and the HIP kernels (libfp8mi.so through fp8_mi355x_lib).

It mirrors the reference's op module fp8_mps_native.py function for function -
same names, same argument meaning, same error behaviour - so that code and
tests written against the reference read the same here:

  fp8_scaled_mm       fp8_mps_native.py:41-95
  fp8_dequantize      fp8_mps_native.py:98-124
  fp8_encode          fp8_mps_native.py:127-155
  fp8_quantize        fp8_mps_native.py:158-190
  fp8_scaled_mm_auto  fp8_mps_native.py:193-210
  fp8_scaled_mm_fast  fp8_mps_native.py:213-267 (kept as an alias: the
                      dequant -> fp16 matmul detour it implemented exists only
                      because Apple GPUs have no FP8 ALU; on gfx950 the MFMA
                      kernel consumes the bytes directly)

What differs, deliberately:
  * the device is "cuda" (PyTorch-ROCm's name for HIP devices), not "mps";
  * kernels are launched on torch's CURRENT stream of the tensor's device and
    never synchronise (the reference's `.item()` in fp8_quantize,
    fp8_mps_native.py:174, is gone: amax, scale and encode all stay on the GPU);
  * bias / scale_result / out_dtype can be passed down and are fused into the
    kernel epilogue (the reference applies them as three extra passes,
    fp8_mps_patch.py:94-104);
  * a per-row scale next to a per-tensor scale is broadcast properly (the
    reference reads out of bounds in that case, fp8_mps_native.py:73 with
    fp8_matmul.metal:144-146);
  * there is no CPU path.  A tensor that is not on a HIP device is moved there
    (as the reference moves to "mps", fp8_mps_native.py:63-66); without a GPU
    that raises;
  * float8_e5m2 is a first-class operand type (the reference decodes e5m2 bytes
    as e4m3, fp8_mps_patch.py:65): fp8_scaled_mm / scaled_mm_colmajor /
    fp8_scaled_mm_auto take each operand's format from its dtype
    (torch.float8_e5m2 -> e5m2; uint8 / float8_e4m3fn -> e4m3) or from the
    keyword-only a_format / b_format for raw bytes, and fp8_encode_e5m2 /
    fp8_dequantize_e5m2 / fp8_quantize_e5m2 are torch's casts.  A call with an
    e5m2 operand has OCP semantics only (NAN_PROPAGATE: inf and NaN bytes are
    values; include/fp8mi.h, fp8mi_scaled_mm_fmt).
"""

from __future__ import annotations

import collections
import threading

import torch

import fp8_mi355x_lib as _l

DEVICE_TYPE = "cuda"  # PyTorch-ROCm reports HIP devices as "cuda"

_DTYPE_CODE = {torch.float32: _l.F32, torch.float16: _l.F16, torch.bfloat16: _l.BF16}
_E4M3 = getattr(torch, "float8_e4m3fn", None)
_E5M2 = getattr(torch, "float8_e5m2", None)


def _operand_format(t: torch.Tensor, given, what: str) -> int:
    """The element format (fp8_mi355x_lib.FMT_*) of a GEMM operand: `given` (the a_format / b_format keyword) when not None,
    else by dtype - torch.float8_e5m2 is e5m2, uint8 and float8_e4m3fn are e4m3."""
    if given is not None:
        if given not in (_l.FMT_E4M3, _l.FMT_E5M2):
            raise AssertionError(f"{what}: unknown operand format {given!r}")
        assert t.element_size() == 1, f"{what}: {t.dtype} is not a one-byte type"
        return given
    if _E5M2 is not None and t.dtype == _E5M2:
        return _l.FMT_E5M2
    assert t.dtype == torch.uint8 or (_E4M3 is not None and t.dtype == _E4M3), f"{what}: {t.dtype} is neither uint8 nor an FP8 dtype"
    return _l.FMT_E4M3

# process-wide defaults; see include/fp8mi.h for the meaning of the modes
NAN_MODE = _l.NAN_ZERO          # reference decode: NaN bytes are 0.0
ENCODE_MODE = _l.ENC_REFERENCE  # reference encode rules


# Conversions made INSIDE this module never involve an fp8 dtype, so they use the C-level Tensor.to: while the
# monkey-patch is installed `tensor.to(...)` is fp8_mps_patch._metal_tensor_to, a Python function that parses the
# overloads of .to before it can decide that the call is none of its business (~3 us per call on the hot path).
_TO = torch._C.TensorBase.to

_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(device):
    """hipStream_t (as int) of torch's current stream on `device`.  The raw accessor skips the construction of a
    torch.cuda.Stream object (1.5 us of the ~4 us this module adds to a call; tools/time_callsite.py)."""
    if _raw_stream is not None:
        return _raw_stream(device.index if device.index is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(device).cuda_stream


class _on_device:
    """`with torch.cuda.device(dev)` only when `dev` is not already current (the context manager costs two device
    switches and ~2 us even when it changes nothing)."""
    __slots__ = ("ctx",)

    def __init__(self, dev):
        self.ctx = None if (dev.index is None or torch.cuda.current_device() == dev.index) else torch.cuda.device(dev)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *exc):
        if self.ctx is not None:
            return self.ctx.__exit__(*exc)
        return False


# split-K workspaces: one per (device, stream) - launches on one stream are ordered, so they can share it; the
# counters at its head are zeroed once here and left zero by every launch (include/fp8mi.h).  Kept alive for the
# life of the process, so a pointer captured into a HIP graph stays valid.
_workspaces: dict = {}
_workspaces_lock = threading.Lock()


def _workspace(device):
    """The split-K workspace of (device, current stream), or None while that stream is being captured into a HIP graph
    and no workspace exists yet: allocating inside a capture would put it into the graph's private pool, where later
    eager launches on the same stream handle would share it (warm the op up once before capturing; without a workspace
    the call simply does not split K)."""
    return _workspace_on(device, _stream(device))


def _workspace_on(device, stream):
    key = (device.index, stream)
    ws = _workspaces.get(key)
    if ws is None:
        if torch.cuda.is_current_stream_capturing():
            return None
        with _workspaces_lock:
            ws = _workspaces.get(key)
            if ws is None:
                ws = torch.empty(int(_l.load().fp8mi_scaled_mm_workspace_bytes()), dtype=torch.uint8, device=device)
                _l.check(_l.load().fp8mi_workspace_reset(ws.data_ptr(), ws.numel(), stream), "fp8mi_workspace_reset")
                _workspaces[key] = ws
    return ws


def reset_workspaces():
    """Zero the arrival counters of every cached split-K workspace (include/fp8mi.h, fp8mi_workspace_reset): only needed
    after a launch was aborted mid-flight (device fault, process-level error recovery) - every completed launch leaves
    them zero by itself."""
    with _workspaces_lock:
        for (dev_index, stream), ws in _workspaces.items():
            with torch.cuda.device(dev_index):
                # a workspace is ordered on the stream it is keyed by: the reset goes onto THAT stream (not the caller's
                # current one), bracketed by device syncs so that it neither races a launch in flight nor trails the next
                torch.cuda.synchronize(dev_index)
                _l.check(_l.load().fp8mi_workspace_reset(ws.data_ptr(), ws.numel(), stream), "fp8mi_workspace_reset")
                torch.cuda.synchronize(dev_index)


def _to_device(t: torch.Tensor) -> torch.Tensor:
    return t if t.device.type == DEVICE_TYPE else t.to(DEVICE_TYPE)


def _scale_arg(scale, device, rows: int, what: str):
    """-> (float32 contiguous tensor on `device`, mode).  1 element = per-tensor,
    `rows` elements (any shape, e.g. (M,1) / (1,N)) = per-row."""
    s = scale
    # already what the kernel reads (the common case: a float32 device scalar or (M,1) / (1,N) column): no new tensor
    if not (s.dtype is torch.float32 and s.device == device and s.is_contiguous()):
        s = _TO(s, device=device, dtype=torch.float32).reshape(-1).contiguous()
    if s.numel() == 1:
        return s, _l.SCALE_TENSOR
    if s.numel() == rows:
        return s, _l.SCALE_ROW
    raise AssertionError(f"{what} has {s.numel()} elements; expected 1 or {rows}")


# ---- what the GEMM functions (tensorwise, MXFP8, MXFP4, blockwise) share around their one ctypes call -----------------------------------

def _operand_rows(t: torch.Tensor, rows: int, K: int):
    """-> (t or its contiguous copy, ld): a GEMM operand's rows must be dense in their K bytes; a padded row stride is fine (no copy)."""
    if not (K == 0 or rows == 0 or (t.stride(1) == 1 and t.stride(0) >= K) or (rows == 1 and t.stride(1) == 1)):
        t = t.contiguous()
    return t, (max(t.stride(0), K) if rows > 1 else max(K, 1))


def _output(out, out_dtype, M: int, N: int, dev):
    """-> (C, out_code, ldc): `out` after its checks, or a new (M, N) tensor of `out_dtype` (float32 by default)."""
    out_dtype = torch.float32 if out_dtype is None else out_dtype
    out_code = _out_code(out_dtype)
    if out is not None:
        assert out.shape == (M, N) and out.dtype == out_dtype and out.device == dev, "out must be (M, N) out_dtype on A's device"
        assert N <= 1 or out.stride(1) == 1, "out needs unit column stride"
        C = out
    else:
        C = torch.empty((M, N), dtype=out_dtype, device=dev)
    return C, out_code, (max(C.stride(0), N) if M > 1 else max(N, 1))


def _epilogue_args(bias, scale_result, transposed_epilogue, M: int, N: int, dev):
    """-> (bias_ptr, bias_code, sr_ptr, keep): the fused epilogue's arguments; `keep` holds the tensors the pointers point into (the caller
    keeps it until the launch is issued).  A tensor the kernel can read as it is - on `dev`, contiguous, a dtype it knows - is not copied."""
    bias_ptr, bias_code = None, _l.F32
    if bias is not None:
        if bias.device != dev:
            bias = _TO(bias, device=dev)
        if bias.dtype not in _DTYPE_CODE:
            bias = _TO(bias, torch.float32)
        if not bias.is_contiguous():
            bias = bias.reshape(-1).contiguous()
        nb = M if transposed_epilogue else N
        assert bias.numel() == nb, f"bias has {bias.numel()} elements; expected {nb}"
        bias_ptr, bias_code = bias.data_ptr(), _DTYPE_CODE[bias.dtype]
    if transposed_epilogue:
        bias_code |= _l.EPILOGUE_TRANSPOSED
    sr_ptr = None
    if scale_result is not None:
        if not (scale_result.dtype is torch.float32 and scale_result.device == dev and scale_result.is_contiguous()):
            scale_result = _TO(scale_result, device=dev, dtype=torch.float32).reshape(-1).contiguous()
        assert scale_result.numel() == 1, "scale_result must have one element"
        sr_ptr = scale_result.data_ptr()
    return bias_ptr, bias_code, sr_ptr, (bias, scale_result)


def _launch_gemm(entry: str, what: str, dev, use_workspace: bool, head: tuple, split_k: int, tail: tuple = ()):
    """The ONE ctypes call: libfp8mi's `entry`(*head, split_k, workspace, workspace_bytes, *tail, stream) on torch's current stream of `dev`.
    use_workspace is the family's own condition for asking for the split-K workspace; without one the call does not split K."""
    fn = getattr(_l.load(), entry)
    with _on_device(dev):
        stream = _stream(dev)
        ws = _workspace_on(dev, stream) if use_workspace else None
        if ws is None:
            rc = fn(*head, 1, None, 0, *tail, stream)
        else:
            rc = fn(*head, split_k, ws.data_ptr(), ws.numel(), *tail, stream)
    if rc:
        _l.check(rc, what)


def fp8_scaled_mm(A: torch.Tensor, B: torch.Tensor, scale_a: torch.Tensor, scale_b: torch.Tensor,
                  *, bias: torch.Tensor | None = None, scale_result: torch.Tensor | None = None,
                  out_dtype: torch.dtype | None = None, nan_mode: int | None = None,
                  kernel: int = _l.KERNEL_AUTO, split_k: int = 0, out: torch.Tensor | None = None,
                  transposed_epilogue: bool = False, a_format: int | None = None, b_format: int | None = None) -> torch.Tensor:
    """FP8 scaled matrix multiplication on the GPU.

    A: (M, K) uint8 - e4m3fn bytes, row-major
    B: (N, K) uint8 - e4m3fn bytes, row-major (i.e. pre-transposed); a row
       stride larger than K is accepted without a copy
    Either may also be a float8_e4m3fn or float8_e5m2 tensor: the format is then
    taken from the dtype; a_format / b_format (fp8_mi355x_lib.FMT_E4M3 /
    FMT_E5M2) give it for raw bytes.  With an e5m2 operand the call runs with
    NAN_PROPAGATE whatever `nan_mode` says (OCP semantics only, include/fp8mi.h).
    scale_a: [1] or [M] float32;  scale_b: [1] or [N] float32
    Returns (M, N) float32 (or `out_dtype`) on the device:
        ((A_dec @ B_dec.T) * scale_a * scale_b + bias) * scale_result
    Same contract as fp8_mps_native.py:41-95 (asserts included); the kernel is
    picked by shape inside the library (GEMV for M == 1, MFMA GEMM otherwise).
    split_k: 0 lets the library slice K when M x N gives too few tiles to fill
    the GPU (small batch, deep K), 1 forbids it, > 1 forces that many slices.
    out: optional (M, N) destination of `out_dtype` with unit column stride (any
    row stride: e.g. a slab of a larger buffer); returned instead of a new tensor.
    transposed_epilogue: the call computes C^T = W . X^T for a caller whose
    activations are `B` here (fp8_sharded_linear): `bias` then has M elements and
    runs along the rows, and the scales are applied in the order of the
    untransposed product (include/fp8mi.h, FP8MI_EPILOGUE_TRANSPOSED).
    """
    if a_format is None and b_format is None and A.dtype == torch.uint8 and B.dtype == torch.uint8:
        fa = fb = _l.FMT_E4M3
    else:
        fa, fb = _operand_format(A, a_format, "A"), _operand_format(B, b_format, "B")
        if A.dtype != torch.uint8:
            A = A.view(torch.uint8)
        if B.dtype != torch.uint8:
            B = B.view(torch.uint8)
    assert A.dim() == 2 and B.dim() == 2
    M, K = A.shape
    N = B.shape[0]
    assert B.shape[1] == K

    A = _to_device(A)
    B = _to_device(B)
    dev = A.device
    assert B.device == dev, "A and B must be on the same device"
    A, lda = _operand_rows(A, M, K)
    B, ldb = _operand_rows(B, N, K)
    # The MFMA / vec-mat kernels read 16-byte pieces: K, lda, ldb multiples of 16 and 16-byte aligned bases.  Anything else the reference
    # accepts (fp8_mps_native.py:55-60 asks for contiguity only: K = 4100, a sliced weight view) would run on the library's generic kernel -
    # one wave per output element, orders of magnitude slower (M=N=4096, K=4100: profiles/r04_unaligned.txt).  Large such problems are
    # copied once per call into aligned buffers whose rows are padded with ZERO bytes up to the next multiple of 16: a zero byte is +0.0
    # in e4m3 - and in e5m2 - so the padded product is the same sum (tests/test_gpu_parity.py::test_unaligned_operands_take_the_padded_mfma_path).
    if kernel == _l.KERNEL_AUTO and K > 0 and M >= 2 and M * N * K >= PAD_MIN_MACS and not (_aligned16(A, M, K, lda) and _aligned16(B, N, K, ldb)):
        A, B, K, lda, ldb = _pad_operands(A, B, M, N, K)
    return _scaled_mm_core(A, B, M, N, K, lda, ldb, dev, scale_a, scale_b, bias, scale_result, out_dtype, nan_mode,
                           kernel, split_k, out, transposed_epilogue, fa, fb)


PAD_MIN_MACS = 1 << 22   # below this many multiply-adds the generic kernel is as fast as two extra copy launches; a single row (M = 1) never pays for
                         # a copy of the whole weight matrix (K=4100 N=4096: generic 22.6 us, padded 33.0: profiles/r04_unaligned.txt)


def _aligned16(t, rows, K, ld):
    return K % 16 == 0 and t.data_ptr() % 16 == 0 and (rows <= 1 or ld % 16 == 0)


def _pad_operands(A, B, M, N, K):
    """-> (A', B', K', lda', ldb'): fresh, contiguous (so 16-byte aligned) copies with rows zero-padded to K' = the next multiple of 16."""
    Kp = (K + 15) // 16 * 16
    if Kp != K:
        pad = torch.nn.functional.pad
        return pad(A, (0, Kp - K)), pad(B, (0, Kp - K)), Kp, Kp, Kp
    return A.contiguous().clone() if A.data_ptr() % 16 else A.contiguous(), B.contiguous().clone() if B.data_ptr() % 16 else B.contiguous(), K, K, K


def _scaled_mm_core(a_keep, b_keep, M, N, K, lda, ldb, dev, scale_a, scale_b, bias, scale_result, out_dtype, nan_mode,
                    kernel, split_k, out, transposed_epilogue, a_format=_l.FMT_E4M3, b_format=_l.FMT_E4M3):
    """Everything behind the operand checks: scales, output, epilogue arguments, ONE ctypes call.  `a_keep` / `b_keep`
    are tensors of ANY dtype whose storage holds the (M,K) / (N,K) byte rows at data_ptr() with row strides lda / ldb
    (the patch hands over the float8 tensors themselves: no uint8 views, no .t()); a_format / b_format say what the bytes
    are.  e4m3 x e4m3 goes through fp8mi_scaled_mm_ws as it always has; an e5m2 operand through fp8mi_scaled_mm_fmt with
    NAN_PROPAGATE."""
    sa, sa_mode = _scale_arg(scale_a, dev, M, "scale_a")
    sb, sb_mode = _scale_arg(scale_b, dev, N, "scale_b")

    C, out_code, ldc = _output(out, out_dtype, M, N, dev)
    if M == 0 or N == 0:
        return C
    bias_ptr, bias_code, sr_ptr, _keep = _epilogue_args(bias, scale_result, transposed_epilogue, M, N, dev)
    e5m2 = not (a_format == _l.FMT_E4M3 and b_format == _l.FMT_E4M3)
    head = (a_keep.data_ptr(), b_keep.data_ptr(), C.data_ptr(), sa.data_ptr(), sb.data_ptr(), bias_ptr, sr_ptr, M, N, K, lda, ldb, ldc, sa_mode, sb_mode,
            out_code, bias_code, _l.NAN_PROPAGATE if e5m2 else (NAN_MODE if nan_mode is None else nan_mode), kernel)
    # a workspace only where split-K can apply: more than one row, K deep enough to slice
    _launch_gemm("fp8mi_scaled_mm_fmt" if e5m2 else "fp8mi_scaled_mm_ws", "fp8mi_scaled_mm", dev, split_k != 1 and M > 1 and K >= 1024, head, split_k,
                 (a_format, b_format) if e5m2 else ())
    return C


def scaled_mm_colmajor(input: torch.Tensor, other: torch.Tensor, scale_a, scale_b, *, bias=None, scale_result=None,
                       out_dtype=None, a_format: int | None = None, b_format: int | None = None):
    """The call torch._scaled_mm makes, without intermediate tensors: `input` (M,K) row-major and `other` (K,N) in the
    column-major layout torch mandates, both float8_e4m3fn or uint8 ON A HIP DEVICE.  `other`'s storage then already is
    the (N,K) row-major operand the kernels read (fp8_mps_patch.py:77-86 makes it with .t().contiguous()), so the
    pointers and strides are passed as they are.  Returns None when the layout is anything else (the caller falls back
    to fp8_scaled_mm, which copies).  float8_e5m2 operands (or a_format / b_format for raw bytes) take the e5m2 kernels."""
    if input.dim() != 2 or other.dim() != 2:
        return None
    M, K = input.shape
    K2, N = other.shape
    if K2 != K or other.device != input.device:
        return None
    sa0, sa1 = input.stride()
    sb0, sb1 = other.stride()
    if not (K == 0 or M == 0 or (sa1 == 1 and sa0 >= K) or (M == 1 and sa1 == 1)):
        return None
    if not (K == 0 or N == 0 or (sb0 == 1 and sb1 >= K) or (N == 1 and sb0 == 1)):
        return None
    lda = max(sa0, K) if M > 1 else max(K, 1)
    ldb = max(sb1, K) if N > 1 else max(K, 1)
    e5 = _E5M2
    if a_format is None and b_format is None and input.dtype != e5 and other.dtype != e5:
        return _scaled_mm_core(input, other, M, N, K, lda, ldb, input.device, scale_a, scale_b, bias, scale_result, out_dtype,
                               None, _l.KERNEL_AUTO, 0, None, False)
    return _scaled_mm_core(input, other, M, N, K, lda, ldb, input.device, scale_a, scale_b, bias, scale_result, out_dtype,
                           None, _l.KERNEL_AUTO, 0, None, False, _operand_format(input, a_format, "input"),
                           _operand_format(other, b_format, "other"))


# ---- what the stand-alone casts and quantisers share around their one ctypes call -----------------------------------------

def _call(entry: str, dev, *args):
    """The ONE ctypes call of a cast: libfp8mi's `entry`(*args, stream) on torch's current stream of `dev`."""
    fn = getattr(_l.load(), entry)
    with _on_device(dev):
        rc = fn(*args, _stream(dev))
    if rc:
        _l.check(rc, entry)


def _rows_view(t: torch.Tensor, any_row_stride: bool = False):
    """-> (2-D tensor, rows, cols, ld): a 2-D view whose last dimension is contiguous (a column slice of a wider tensor) is used in
    place through its row stride; anything else is made contiguous and flattened to (rows, cols).  any_row_stride: a row stride below
    cols is no reason for a copy (the 2-D quantisers and dequantisers; the library then sees ld = cols)."""
    if t.dim() == 2 and t.is_contiguous():   # (the common case, ahead of the stride arithmetic: dense rows, ld = cols)
        rows, cols = t.shape
        return t, rows, cols, max(cols, 1)
    cols = t.shape[-1]
    if not (t.dim() == 2 and (t.stride(1) == 1 or cols <= 1) and (any_row_stride or t.shape[0] <= 1 or t.stride(0) >= cols)):
        t = t.contiguous().reshape(-1, cols)
    rows = t.shape[0]
    return t, rows, cols, (max(t.stride(0), cols, 1) if rows > 1 else max(cols, 1))


def _scalar_ptr(scale, dev, what: str):
    """-> (pointer, the float32 tensor on `dev` it points into) of a one-element scale, (None, None) without one"""
    if scale is None:
        return None, None
    scale = _TO(scale, device=dev, dtype=torch.float32).reshape(-1).contiguous()
    assert scale.numel() == 1, f"{what} must be a scalar"
    return scale.data_ptr(), scale


def _out_code(out_dtype) -> int:
    code = _DTYPE_CODE.get(out_dtype)
    if code is None:
        raise AssertionError(f"unsupported out_dtype {out_dtype}")
    return code


def _float_source(x: torch.Tensor) -> torch.Tensor:
    """a quantiser's input on the device, in a dtype the kernels read (ints, float64 ...: converted to float32)"""
    x = _to_device(x)
    return x if x.dtype in _DTYPE_CODE else _TO(x, torch.float32)


def fp8_dequantize(input: torch.Tensor, scale: torch.Tensor | None = None,
                   out_dtype: torch.dtype = torch.float16) -> torch.Tensor:
    """FP8 -> half dequantisation on the GPU (fp8_mps_native.py:98-124).

    input: uint8 tensor (e4m3fn bytes);  scale: scalar tensor or None.
    Returns float16 (or `out_dtype`) of the same shape:
    half(decode(b)) * half(scale), the product formed in float16 as in the
    reference; float32 / bfloat16 outputs convert that half value.
    """
    input = _to_device(input)
    assert input.dtype == torch.uint8
    dev = input.device
    src = input.contiguous()
    out = torch.empty(input.shape, dtype=out_dtype, device=dev)
    if src.numel() == 0:
        return out
    s_ptr, _keep = _scalar_ptr(scale, dev, "scale")
    _call("fp8mi_dequant", dev, src.data_ptr(), out.data_ptr(), s_ptr, src.numel(), _DTYPE_CODE[out_dtype])
    return out


def _encode_source(input: torch.Tensor, result: bool = True):
    """-> (the flat casts' source: on the device, a dtype the kernels read, contiguous; its dtype code; result: an empty uint8 tensor of its shape)"""
    inp = _float_source(input).contiguous()   # (ints, float64 ...: the reference converts to float32 first)
    return inp, _DTYPE_CODE[inp.dtype], (torch.empty(inp.shape, dtype=torch.uint8, device=inp.device) if result else None)


def fp8_encode(input: torch.Tensor, encode_mode: int | None = None) -> torch.Tensor:
    """Float -> FP8 bytes without scaling (fp8_mps_native.py:127-155): values
    keep their magnitude, saturating at +-448.  Used by .to(float8_e4m3fn) and
    .copy_().  float16 / bfloat16 sources are widened inside the kernel.
    Returns uint8 of the same shape."""
    inp, code, out = _encode_source(input)
    if inp.numel() == 0:
        return out
    _call("fp8mi_encode", inp.device, inp.data_ptr(), code, out.data_ptr(), None, inp.numel(), ENCODE_MODE if encode_mode is None else encode_mode)
    return out


def fp8_quantize(input: torch.Tensor, encode_mode: int | None = None):
    """Float -> FP8 with automatic amax scaling (fp8_mps_native.py:158-190).

    Returns (uint8 tensor, inverse_scale[1] float32) with
    scale = 448 / max|input|; everything (amax, scale, encode) runs on the
    device, no host read-back."""
    inp, code, out = _encode_source(input)
    scales = torch.empty(2, dtype=torch.float32, device=inp.device)
    _call("fp8mi_quantize", inp.device, inp.data_ptr(), code, out.data_ptr(), scales.data_ptr(), inp.numel(),
          ENCODE_MODE if encode_mode is None else encode_mode)
    return out, scales[1:2]


def _linear_out_dtype(x: torch.Tensor, K: int, out_dtype, weight: str = "weight"):
    """The frame of the *_linear_* / *_mlp_* functions: x's features checked against the weight's K; -> out_dtype, by default x's
    (float32 for other inputs).  The result goes back to x's leading dimensions with _like_rows_of."""
    assert x.shape[-1] == K, f"x has {x.shape[-1]} features; {weight} expects {K}"
    if out_dtype is None:
        return x.dtype if x.dtype in _DTYPE_CODE else torch.float32
    return out_dtype


def _like_rows_of(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    return y.reshape(*x.shape[:-1], y.shape[-1])


def fp8_linear(x: torch.Tensor, weight_u8: torch.Tensor, weight_scale: torch.Tensor, bias: torch.Tensor | None = None,
               out_dtype: torch.dtype | None = None, weight_format: int | None = None) -> torch.Tensor:
    """y = x @ dequant(W).T + bias with dynamic per-tensor activation quantisation - the composition the reference's
    call sites perform around its two entry points (fp8_quantize, fp8_mps_native.py:158-190, then torch._scaled_mm
    through fp8_mps_patch.py:53-106), as one call: amax + scaled encode of x (two launches, no host sync), then the
    scaled matmul with the fused bias / cast epilogue.

    x: (..., K) float32 / float16 / bfloat16;  weight_u8: (N, K) e4m3fn bytes;  weight_scale: [1] or [N] float32.
    An fp8_e5m2 checkpoint's weight goes in as a float8_e5m2 tensor or as bytes with weight_format=FMT_E5M2 (the
    activations are still quantised to e4m3; the product then has OCP NaN semantics).
    Returns (..., N) in `out_dtype` (default: x.dtype, float32 for other inputs)."""
    return _dense_linear("tensor", x, weight_u8, weight_scale, bias, out_dtype, weight_format)


# ---- float8_e5m2 casts (OCP / torch semantics; include/fp8mi.h) -----------------------------------------------------------------

def fp8_encode_e5m2(input: torch.Tensor, prescale: torch.Tensor | None = None) -> torch.Tensor:
    """Float -> float8_e5m2, byte for byte torch's CPU `x.to(torch.float8_e5m2)` (RNE, overflow -> +-inf, NaN -> 0x7F | sign),
    of `input * prescale` (a one-element float32 tensor, the product rounded to float32 first) when a prescale is given.
    Returns a float8_e5m2 tensor of the same shape."""
    inp, code, out = _encode_source(input)
    if inp.numel() == 0:
        return out.view(_E5M2)
    ps_ptr, _keep = _scalar_ptr(prescale, inp.device, "prescale")
    _call("fp8mi_encode_e5m2", inp.device, inp.data_ptr(), code, out.data_ptr(), ps_ptr, inp.numel())
    return out.view(_E5M2)


def fp8_dequantize_e5m2(input: torch.Tensor, scale: torch.Tensor | None = None, out_dtype: torch.dtype = torch.float16) -> torch.Tensor:
    """float8_e5m2 (or its uint8 bytes) -> out_dtype: cast(float(dec(b)) * scale), the product in float32 rounded once; inf and
    NaN are preserved.  scale: a one-element tensor or None."""
    input = _to_device(input)
    assert input.dtype == torch.uint8 or input.dtype == _E5M2, f"expected float8_e5m2 or uint8 bytes, got {input.dtype}"
    dev = input.device
    src = input.contiguous()
    out = torch.empty(input.shape, dtype=out_dtype, device=dev)
    if src.numel() == 0:
        return out
    s_ptr, _keep = _scalar_ptr(scale, dev, "scale")
    _call("fp8mi_dequant_e5m2", dev, src.data_ptr(), out.data_ptr(), s_ptr, src.numel(), _DTYPE_CODE[out_dtype])
    return out


def fp8_quantize_e5m2(input: torch.Tensor):
    """Float -> float8_e5m2 with amax scaling, on the device without a host read-back: scale = 57344 / max|input| (1 for an
    all-zero input), q = e5m2_rne(clamp(input * scale, +-57344)).  Returns (float8_e5m2 tensor, inverse_scale[1] float32)
    - the inverse scale is what _scaled_mm consumes."""
    inp, code, out = _encode_source(input)
    scales = torch.empty(2, dtype=torch.float32, device=inp.device)
    _call("fp8mi_quantize_e5m2", inp.device, inp.data_ptr(), code, out.data_ptr(), scales.data_ptr(), inp.numel())
    return out.view(_E5M2), scales[1:2]


# ---- MXFP8: one E8M0 scale (torch.float8_e8m0fnu, 2^(s - 127)) per 32 elements of a row (include/fp8mi.h) ------------------

_E8M0 = getattr(torch, "float8_e8m0fnu", None)
_FP4X2 = getattr(torch, "float4_e2m1fn_x2", None)
# the block-scaled forms of the ring tile kernels (include/fp8mi.h, fp8mi_scaled_mm_mxfp8); GENERIC and AUTO are accepted too
MXFP8_KERNELS = (_l.KERNEL_GEMM_128, _l.KERNEL_GEMM_128x64, _l.KERNEL_GEMM_64x128, _l.KERNEL_GEMM_64x64,
                 _l.KERNEL_GEMM_32x64, _l.KERNEL_GEMM_32x32, _l.KERNEL_GEMM_128D)


def _e8m0_bytes(scale: torch.Tensor) -> torch.Tensor:
    if _E8M0 is not None and scale.dtype == _E8M0:
        return scale.view(torch.uint8)
    assert scale.dtype == torch.uint8, f"MXFP8 scales are float8_e8m0fnu (or their uint8 bytes), not {scale.dtype}"
    return scale


def mxfp8_scale_ld(scale: torch.Tensor, rows: int, K: int):
    """The row stride (bytes) at which `scale` holds the (rows, K/32) E8M0 block scales of an operand, or None if it holds no
    such layout.  Accepted: a 2-D (rows', cols') tensor with unit column stride, rows' >= rows and cols' >= K/32 (this covers
    torch's padded (128 * ceil(rows/128), round_up(K/32, 4)) allocation), or a flat tensor of exactly rows * K/32 elements or of
    that padded size.  Plain row-major order: the blocked (swizzled) layout of cuBLAS is not read."""
    nb = K // 32
    if scale.dim() == 2:
        r, c = scale.shape
        if r >= rows and c >= nb and (rows == 0 or nb == 0):   # no scale is read: an empty tensor's strides are arbitrary
            return max(c, nb)
        if r >= rows and c >= nb and (scale.stride(1) == 1 or c == 1) and (rows <= 1 or scale.stride(0) >= nb):
            return max(scale.stride(0), nb) if rows > 1 else max(c, nb)
        return None
    n = scale.numel()
    if scale.dim() <= 1 and (scale.dim() == 0 or scale.stride(0) == 1):
        if n == rows * nb:
            return nb
        padded = (rows + 127) // 128 * 128 * ((nb + 3) // 4 * 4)
        if n == padded and n > 0:
            return (nb + 3) // 4 * 4
    return None


def _mx_scales(scale, rows, K, dev, what):
    """-> (uint8 tensor on dev whose storage holds the scales, ld).  The matrix-core kernels read scales in 4-byte K-steps: a row
    stride that is not a multiple of 4 (or an unaligned base) is copied once into torch's padded layout."""
    s = _e8m0_bytes(scale)
    if s.device != dev:
        s = _TO(s, device=dev)
    ld = mxfp8_scale_ld(s, rows, K)
    if ld is None:
        raise AssertionError(f"{what}: {tuple(scale.shape)} E8M0 scales do not hold a ({rows}, {K // 32}) row-major block-scale layout")
    nb = K // 32
    if nb > 0 and (ld % 4 or s.data_ptr() % 4):
        ldp = (nb + 3) // 4 * 4
        buf = torch.full((rows, ldp), 0x7F, dtype=torch.uint8, device=dev)
        buf[:, :nb].copy_(torch.as_strided(s, (rows, nb), (ld, 1)))
        return buf, ldp
    return s, max(ld, 1)


def fp8_scaled_mm_mxfp8(A: torch.Tensor, B: torch.Tensor, scale_a: torch.Tensor, scale_b: torch.Tensor,
                        *, bias: torch.Tensor | None = None, scale_result: torch.Tensor | None = None,
                        out_dtype: torch.dtype | None = None, nan_mode: int | None = None,
                        kernel: int = _l.KERNEL_AUTO, split_k: int = 0, out: torch.Tensor | None = None,
                        transposed_epilogue: bool = False) -> torch.Tensor:
    """MXFP8 (block-scaled) matrix multiplication on the GPU.

    A: (M, K) e4m3fn bytes (uint8 or float8_e4m3fn), row-major;  B: (N, K) the same (row stride >= K accepted)
    scale_a: (M, K/32) E8M0 scales (float8_e8m0fnu or uint8), scale_b: (N, K/32) - row-major, padded allocations accepted
    (mxfp8_scale_ld).  K must be a multiple of 32.  Returns (M, N) float32 (or `out_dtype`):
        (sum_blocks 2^(sa-127) 2^(sb-127) sum_k dec(a) dec(b) + bias) * scale_result
    kernel: AUTO, GENERIC or one of MXFP8_KERNELS; split_k, out and transposed_epilogue as in fp8_scaled_mm."""
    assert A.dim() == 2 and B.dim() == 2 and A.element_size() == 1 and B.element_size() == 1
    M, K = A.shape
    N = B.shape[0]
    assert B.shape[1] == K
    assert K % 32 == 0, f"K={K}: MXFP8 needs a multiple of the 32-element scale block"
    A = _to_device(A)
    B = _to_device(B)
    dev = A.device
    assert B.device == dev, "A and B must be on the same device"
    A, lda = _operand_rows(A, M, K)
    B, ldb = _operand_rows(B, N, K)
    sa, ld_sa = _mx_scales(scale_a, M, K, dev, "scale_a")
    sb, ld_sb = _mx_scales(scale_b, N, K, dev, "scale_b")
    C, out_code, ldc = _output(out, out_dtype, M, N, dev)
    if M == 0 or N == 0:
        return C
    bias_ptr, bias_code, sr_ptr, _keep = _epilogue_args(bias, scale_result, transposed_epilogue, M, N, dev)
    _launch_gemm("fp8mi_scaled_mm_mxfp8", "fp8mi_scaled_mm_mxfp8", dev, split_k != 1 and K >= 1024,
                 (A.data_ptr(), B.data_ptr(), C.data_ptr(), sa.data_ptr(), ld_sa, sb.data_ptr(), ld_sb, bias_ptr, sr_ptr, M, N, K, lda, ldb, ldc, out_code,
                  bias_code, NAN_MODE if nan_mode is None else nan_mode, kernel), split_k)
    return C


# the stand-alone MX quantisers and dequantisers over their two element formats: elements per byte, the packed matrix's dtype, the word in the assertion
_MX_ELEMENTS = {"mxfp8": (1, None, "MXFP8"), "mxfp4": (2, _FP4X2, "MXFP4")}


def _e8m0_operand(scales: torch.Tensor, rows: int, cols: int, dev):
    """-> (uint8 tensor on dev, ld_s): the (rows, ceil(cols / 32)) E8M0 scales of a dequantiser, read in place through their row stride"""
    s = _e8m0_bytes(scales)
    if s.device != dev:
        s = _TO(s, device=dev)
    nb = (cols + 31) // 32
    ld_s = mxfp8_scale_ld(s, rows, nb * 32)
    if ld_s is None:
        raise AssertionError(f"scales {tuple(scales.shape)} do not hold ({rows}, {nb}) block scales")
    return s, max(ld_s, 1)


def _quantize_mx(fmt: str, x: torch.Tensor):
    per_byte, packed, word = _MX_ELEMENTS[fmt]
    x = _float_source(x)
    cols = x.shape[-1]
    assert cols % 32 == 0, f"{cols} columns: {word} needs a multiple of 32"
    x2, rows, cols, ld_in = _rows_view(x.reshape(-1, cols) if x.dim() != 2 else x, True)
    dev = x2.device
    q = torch.empty((rows, cols // per_byte), dtype=torch.uint8, device=dev)
    sc = torch.empty((rows, cols // 32), dtype=torch.uint8, device=dev)
    _call(f"fp8mi_quantize_{fmt}", dev, x2.data_ptr(), _DTYPE_CODE[x2.dtype], rows, cols, ld_in, q.data_ptr(), max(cols // per_byte, 1), sc.data_ptr(),
          max(cols // 32, 1))
    q = q if packed is None else q.view(packed)
    return q.reshape(*x.shape[:-1], cols // per_byte), (sc.view(_E8M0) if _E8M0 is not None else sc).reshape(*x.shape[:-1], cols // 32)


def _dequantize_mx(fmt: str, q: torch.Tensor, scales: torch.Tensor, out_dtype: torch.dtype) -> torch.Tensor:
    per_byte = _MX_ELEMENTS[fmt][0]
    q = _to_device(q)
    q, rows, cb, ld_in = _rows_view(q, True)
    cols, dev = per_byte * cb, q.device
    s, ld_s = _e8m0_operand(scales, rows, cols, dev)
    out_code = _out_code(out_dtype)
    out = torch.empty((rows, cols), dtype=out_dtype, device=dev)
    _call(f"fp8mi_dequant_{fmt}", dev, q.data_ptr(), rows, cols, ld_in, s.data_ptr(), ld_s, out.data_ptr(), out_code)
    return out


def fp8_quantize_mxfp8(x: torch.Tensor):
    """(rows, cols) float32 / float16 / bfloat16 (row stride >= cols accepted; cols % 32 == 0) -> (q, scales):
    q (rows, cols) uint8 e4m3fn bytes, scales (rows, cols/32) float8_e8m0fnu - byte for byte torch's MXFP8 recipe
    (to_mxfp(x, 32, "mxfp8"), include/fp8mi.h).  Any leading dimensions are folded into rows."""
    return _quantize_mx("mxfp8", x)


def fp8_dequantize_mxfp8(q: torch.Tensor, scales: torch.Tensor, out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """(rows, cols) e4m3fn bytes and their (rows, ceil(cols/32)) E8M0 scales -> dec(q) * 2^(s - 127) as out_dtype (OCP decode:
    NaN bytes and the NaN scale 0xFF give NaN)."""
    assert q.dim() == 2 and q.element_size() == 1
    return _dequantize_mx("mxfp8", q, scales, out_dtype)


def fp8_linear_mxfp8(x: torch.Tensor, w_q: torch.Tensor, w_scales: torch.Tensor, bias: torch.Tensor | None = None,
                     out_dtype: torch.dtype | None = None) -> torch.Tensor:
    """y = x @ dequant_mxfp8(W).T + bias with dynamic MXFP8 quantisation of the activations (one scale per 32 features of
    every row) - the block-scaled counterpart of fp8_linear.

    x: (..., K) float32 / float16 / bfloat16 (K % 32 == 0);  w_q: (N, K) e4m3fn bytes;  w_scales: (N, K/32) E8M0
    (fp8_quantize_mxfp8 of the weight).  Returns (..., N) in `out_dtype` (default: x.dtype, float32 for other inputs)."""
    return _dense_linear("mxfp8", x, w_q, w_scales, bias, out_dtype)


# ---- MXFP4: two e2m1 codes per byte (torch.float4_e2m1fn_x2, the even element in the low nibble), one E8M0 scale per 32 elements

# the MXFP4 forms of the ring tile kernels (include/fp8mi.h, fp8mi_scaled_mm_mxfp4): the same tiles as MXFP8_KERNELS
MXFP4_KERNELS = MXFP8_KERNELS


def _fp4_bytes(t: torch.Tensor) -> torch.Tensor:
    if _FP4X2 is not None and t.dtype == _FP4X2:
        return t.view(torch.uint8)
    assert t.dtype == torch.uint8, f"MXFP4 operands are float4_e2m1fn_x2 (or their uint8 bytes), not {t.dtype}"
    return t


def fp8_scaled_mm_mxfp4(A: torch.Tensor, B: torch.Tensor, scale_a: torch.Tensor, scale_b: torch.Tensor,
                        *, bias: torch.Tensor | None = None, scale_result: torch.Tensor | None = None,
                        out_dtype: torch.dtype | None = None, kernel: int = _l.KERNEL_AUTO, split_k: int = 0,
                        out: torch.Tensor | None = None, transposed_epilogue: bool = False) -> torch.Tensor:
    """MXFP4 (e2m1 x e2m1, block-scaled) matrix multiplication on the GPU.

    A: (M, K/2) float4_e2m1fn_x2 (or uint8) - two e2m1 codes per byte, row-major;  B: (N, K/2) the same (row stride >= K/2
    accepted).  scale_a: (M, K/32) E8M0 scales (float8_e8m0fnu or uint8), scale_b: (N, K/32), layouts as in fp8_scaled_mm_mxfp8.
    K = 2 x A.shape[1] must be a multiple of 32.  Returns (M, N) float32 (or `out_dtype`):
        (sum_blocks 2^(sa-127) 2^(sb-127) sum_k e2m1(a) e2m1(b) + bias) * scale_result
    kernel: AUTO, GENERIC or one of MXFP4_KERNELS; split_k, out and transposed_epilogue as in fp8_scaled_mm."""
    assert A.dim() == 2 and B.dim() == 2
    A, B = _fp4_bytes(A), _fp4_bytes(B)
    M, Kb = A.shape
    N = B.shape[0]
    assert B.shape[1] == Kb
    K = 2 * Kb
    assert K % 32 == 0, f"K={K}: MXFP4 needs a multiple of the 32-element scale block"
    A = _to_device(A)
    B = _to_device(B)
    dev = A.device
    assert B.device == dev, "A and B must be on the same device"
    A, lda = _operand_rows(A, M, Kb)
    B, ldb = _operand_rows(B, N, Kb)
    sa, ld_sa = _mx_scales(scale_a, M, K, dev, "scale_a")
    sb, ld_sb = _mx_scales(scale_b, N, K, dev, "scale_b")
    C, out_code, ldc = _output(out, out_dtype, M, N, dev)
    if M == 0 or N == 0:
        return C
    bias_ptr, bias_code, sr_ptr, _keep = _epilogue_args(bias, scale_result, transposed_epilogue, M, N, dev)
    _launch_gemm("fp8mi_scaled_mm_mxfp4", "fp8mi_scaled_mm_mxfp4", dev, split_k != 1 and Kb >= 1024,
                 (A.data_ptr(), B.data_ptr(), C.data_ptr(), sa.data_ptr(), ld_sa, sb.data_ptr(), ld_sb, bias_ptr, sr_ptr, M, N, K, lda, ldb, ldc, out_code,
                  bias_code, kernel), split_k)
    return C


def fp8_quantize_mxfp4(x: torch.Tensor):
    """(rows, cols) float32 / float16 / bfloat16 (row stride >= cols accepted; cols % 32 == 0) -> (q, scales):
    q (rows, cols/2) float4_e2m1fn_x2 (uint8 where torch lacks the dtype), scales (rows, cols/32) float8_e8m0fnu - byte for byte
    torch's MXFP4 recipe (to_mxfp(x, 32, "mxfp4"), include/fp8mi.h).  Any leading dimensions are folded into rows."""
    return _quantize_mx("mxfp4", x)


def fp8_dequantize_mxfp4(q: torch.Tensor, scales: torch.Tensor, out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """(rows, cols/2) e2m1 pairs (float4_e2m1fn_x2 or uint8) and their (rows, ceil(cols/32)) E8M0 scales -> (rows, cols)
    e2m1 x 2^(s - 127) as out_dtype (the NaN scale 0xFF gives NaN)."""
    assert q.dim() == 2
    return _dequantize_mx("mxfp4", _fp4_bytes(q), scales, out_dtype)


def fp8_linear_mxfp4(x: torch.Tensor, w_q: torch.Tensor, w_scales: torch.Tensor, bias: torch.Tensor | None = None,
                     out_dtype: torch.dtype | None = None) -> torch.Tensor:
    """y = x @ dequant_mxfp4(W).T + bias with dynamic MXFP4 quantisation of the activations (one scale per 32 features of
    every row) - the e2m1 counterpart of fp8_linear_mxfp8.

    x: (..., K) float32 / float16 / bfloat16 (K % 32 == 0);  w_q: (N, K/2) e2m1 pairs;  w_scales: (N, K/32) E8M0
    (fp8_quantize_mxfp4 of the weight).  Returns (..., N) in `out_dtype` (default: x.dtype, float32 for other inputs)."""
    return _dense_linear("mxfp4", x, w_q, w_scales, bias, out_dtype)


# ---- MXW4A8: e4m3 activations (fp8_quantize_mxfp8's bytes) against e2m1 weights (fp8_quantize_mxfp4's pairs), E8M0 scales on both sides

# the MXW4A8 forms of the ring tile kernels (include/fp8mi.h, fp8mi_scaled_mm_mxw4a8): the same tiles as MXFP8_KERNELS
MXW4A8_KERNELS = MXFP8_KERNELS


def fp8_scaled_mm_mxw4a8(A: torch.Tensor, B: torch.Tensor, scale_a: torch.Tensor, scale_b: torch.Tensor,
                         *, bias: torch.Tensor | None = None, scale_result: torch.Tensor | None = None,
                         out_dtype: torch.dtype | None = None, nan_mode: int | None = None,
                         kernel: int = _l.KERNEL_AUTO, split_k: int = 0, out: torch.Tensor | None = None,
                         transposed_epilogue: bool = False) -> torch.Tensor:
    """MXW4A8 (e4m3 x e2m1, block-scaled) matrix multiplication on the GPU.

    A: (M, K) e4m3fn bytes (uint8 or float8_e4m3fn), row-major;  B: (N, K/2) float4_e2m1fn_x2 (or uint8) - two e2m1 codes per byte (row
    strides >= K and >= K/2 accepted).  scale_a: (M, K/32) E8M0 scales (float8_e8m0fnu or uint8), scale_b: (N, K/32), layouts as in
    fp8_scaled_mm_mxfp8.  K must be a multiple of 32.  Returns (M, N) float32 (or `out_dtype`):
        (sum_blocks 2^(sa-127) 2^(sb-127) sum_k e4m3(a) e2m1(b) + bias) * scale_result
    nan_mode applies to A alone (e2m1 has no NaN encoding).  kernel: AUTO, GENERIC or one of MXW4A8_KERNELS; split_k, out and
    transposed_epilogue as in fp8_scaled_mm."""
    assert A.dim() == 2 and B.dim() == 2 and A.element_size() == 1
    B = _fp4_bytes(B)
    M, K = A.shape
    N = B.shape[0]
    assert 2 * B.shape[1] == K, f"B holds {2 * B.shape[1]} e2m1 elements per row; A has K={K}"
    assert K % 32 == 0, f"K={K}: MXW4A8 needs a multiple of the 32-element scale block"
    A = _to_device(A)
    B = _to_device(B)
    dev = A.device
    assert B.device == dev, "A and B must be on the same device"
    A, lda = _operand_rows(A, M, K)
    B, ldb = _operand_rows(B, N, K // 2)
    sa, ld_sa = _mx_scales(scale_a, M, K, dev, "scale_a")
    sb, ld_sb = _mx_scales(scale_b, N, K, dev, "scale_b")
    C, out_code, ldc = _output(out, out_dtype, M, N, dev)
    if M == 0 or N == 0:
        return C
    bias_ptr, bias_code, sr_ptr, _keep = _epilogue_args(bias, scale_result, transposed_epilogue, M, N, dev)
    _launch_gemm("fp8mi_scaled_mm_mxw4a8", "fp8mi_scaled_mm_mxw4a8", dev, split_k != 1 and K >= 2048,
                 (A.data_ptr(), B.data_ptr(), C.data_ptr(), sa.data_ptr(), ld_sa, sb.data_ptr(), ld_sb, bias_ptr, sr_ptr, M, N, K, lda, ldb, ldc, out_code,
                  bias_code, NAN_MODE if nan_mode is None else nan_mode, kernel), split_k)
    return C


def fp8_linear_mxw4a8(x: torch.Tensor, w_q: torch.Tensor, w_scales: torch.Tensor, bias: torch.Tensor | None = None,
                      out_dtype: torch.dtype | None = None) -> torch.Tensor:
    """y = x @ dequant_mxfp4(W).T + bias with dynamic MXFP8 quantisation of the activations: an MXFP4 checkpoint's weights as they are,
    the activations at e4m3 precision.

    x: (..., K) float32 / float16 / bfloat16 (K % 32 == 0);  w_q: (N, K/2) e2m1 pairs;  w_scales: (N, K/32) E8M0
    (fp8_quantize_mxfp4 of the weight).  Returns (..., N) in `out_dtype` (default: x.dtype, float32 for other inputs)."""
    return _dense_linear("mxw4a8", x, w_q, w_scales, bias, out_dtype)


# ---- blockwise: one fp32 scale per 128 k of every row ("1x128") or of every 128-row block ("128x128") (include/fp8mi.h) -----

# the blockwise forms of the ring tile kernels (fp8mi_scaled_mm_blockwise): the same tiles as MXFP8_KERNELS; GENERIC and AUTO too
BLOCKWISE_KERNELS = MXFP8_KERNELS


def _bw_scales(scale: torch.Tensor, rows: int, K: int, block: int, dev, what: str):
    """-> (float32 tensor on dev, stride_row, stride_k): the (ceil(rows / block), ceil(K / 128)) scales of an operand, read in
    place through their strides (any layout: row-major, torch's outer-dim-major, a transposed view); other dtypes are converted."""
    assert block in (1, 128), f"{what}: block must be 1 or 128, not {block}"
    shape = ((rows + block - 1) // block, (K + 127) // 128)
    assert scale.dim() == 2 and tuple(scale.shape) == shape, f"{what}: {tuple(scale.shape)} scales; expected {shape}"
    s = scale
    if not (s.dtype is torch.float32 and s.device == dev):
        s = _TO(s, device=dev, dtype=torch.float32)
    return s, s.stride(0), s.stride(1)


def fp8_scaled_mm_blockwise(A: torch.Tensor, B: torch.Tensor, scale_a: torch.Tensor, scale_b: torch.Tensor,
                            *, block_a: int = 1, block_b: int = 128, bias: torch.Tensor | None = None,
                            scale_result: torch.Tensor | None = None, out_dtype: torch.dtype | None = None,
                            nan_mode: int | None = None, kernel: int = _l.KERNEL_AUTO, split_k: int = 0,
                            out: torch.Tensor | None = None, transposed_epilogue: bool = False) -> torch.Tensor:
    """Blockwise-scaled FP8 matrix multiplication on the GPU (DeepSeek-style 1x128 / 128x128 scales).

    A: (M, K) e4m3fn bytes (uint8 or float8_e4m3fn), row-major;  B: (N, K) the same (row stride >= K accepted)
    scale_a: (ceil(M / block_a), ceil(K / 128)) float32;  scale_b: (ceil(N / block_b), ceil(K / 128)) float32, any strides (read
    in place: torch's (K/128, N/128) weight scales pass as `.t()`).  Returns (M, N) float32 (or `out_dtype`):
        (sum_b sa(m, b) sb(n, b) sum_{k in block b} dec(a) dec(b) + bias) * scale_result
    kernel: AUTO, GENERIC or one of BLOCKWISE_KERNELS; split_k, out and transposed_epilogue as in fp8_scaled_mm."""
    assert A.dim() == 2 and B.dim() == 2 and A.element_size() == 1 and B.element_size() == 1
    M, K = A.shape
    N = B.shape[0]
    assert B.shape[1] == K
    A = _to_device(A)
    B = _to_device(B)
    dev = A.device
    assert B.device == dev, "A and B must be on the same device"
    A, lda = _operand_rows(A, M, K)
    B, ldb = _operand_rows(B, N, K)
    sa, sa_sr, sa_sk = _bw_scales(scale_a, M, K, block_a, dev, "scale_a")
    sb, sb_sr, sb_sk = _bw_scales(scale_b, N, K, block_b, dev, "scale_b")
    C, out_code, ldc = _output(out, out_dtype, M, N, dev)
    if M == 0 or N == 0:
        return C
    bias_ptr, bias_code, sr_ptr, _keep = _epilogue_args(bias, scale_result, transposed_epilogue, M, N, dev)
    _launch_gemm("fp8mi_scaled_mm_blockwise", "fp8mi_scaled_mm_blockwise", dev, split_k != 1 and K >= 1024,
                 (A.data_ptr(), B.data_ptr(), C.data_ptr(), sa.data_ptr(), sa_sr, sa_sk, block_a, sb.data_ptr(), sb_sr, sb_sk, block_b, bias_ptr, sr_ptr,
                  M, N, K, lda, ldb, ldc, out_code, bias_code, NAN_MODE if nan_mode is None else nan_mode, kernel), split_k)
    return C


def fp8_quantize_blockwise(x: torch.Tensor, block_rows: int = 1):
    """(rows, cols) float32 / float16 / bfloat16 (row stride >= cols accepted) -> (q, scales): q (rows, cols) uint8 e4m3fn bytes,
    scales (ceil(rows / block_rows), ceil(cols / 128)) float32 row-major, one per block of block_rows (1 or 128) x 128 columns:
    s = amax / 448 (1 when that quotient is 0: an all-zero block, or an f32 amax so small that the division underflows),
    q = e4m3_rne(clamp(x / s, -448, 448)) (include/fp8mi.h, tests/blockwise_ref.py)."""
    assert block_rows in (1, 128), f"block_rows must be 1 or 128, not {block_rows}"
    x = _float_source(x)
    assert x.dim() == 2, "blockwise quantisation takes a (rows, cols) matrix"
    x, rows, cols, ld_in = _rows_view(x, True)
    dev = x.device
    nrb, ncb = (rows + block_rows - 1) // block_rows, (cols + 127) // 128
    q = torch.empty((rows, cols), dtype=torch.uint8, device=dev)
    sc = torch.empty((nrb, ncb), dtype=torch.float32, device=dev)
    _call("fp8mi_quantize_blockwise", dev, x.data_ptr(), _DTYPE_CODE[x.dtype], rows, cols, ld_in, block_rows, q.data_ptr(), max(cols, 1), sc.data_ptr(),
          max(ncb, 1), 1)
    return q, sc


def fp8_dequantize_blockwise(q: torch.Tensor, scales: torch.Tensor, block_rows: int = 1, out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """(rows, cols) e4m3fn bytes and their (ceil(rows / block_rows), ceil(cols / 128)) float32 scales (any strides) -> dec(q) * s
    as out_dtype (OCP decode: NaN bytes give NaN; the product in fp32, rounded once to out_dtype)."""
    assert q.dim() == 2 and q.element_size() == 1
    q = _to_device(q)
    q, rows, cols, ld_in = _rows_view(q, True)
    dev = q.device
    s, s_sr, s_sk = _bw_scales(scales, rows, cols, block_rows, dev, "scales")
    out_code = _out_code(out_dtype)
    out = torch.empty((rows, cols), dtype=out_dtype, device=dev)
    _call("fp8mi_dequant_blockwise", dev, q.data_ptr(), rows, cols, ld_in, block_rows, s.data_ptr(), s_sr, s_sk, out.data_ptr(), out_code)
    return out


def fp8_linear_blockwise(x: torch.Tensor, w_q: torch.Tensor, w_scales: torch.Tensor, bias: torch.Tensor | None = None,
                         out_dtype: torch.dtype | None = None) -> torch.Tensor:
    """y = x @ dequant_blockwise(W).T + bias - the DeepSeek linear: dynamic 1x128 quantisation of the activations (one fp32 scale
    per 128 features of every row), then the GEMM against 128x128 weight scales.

    x: (..., K) float32 / float16 / bfloat16;  w_q: (N, K) e4m3fn bytes;  w_scales: (ceil(N/128), ceil(K/128)) float32
    (fp8_quantize_blockwise(W, 128), or a checkpoint's weight_scale_inv).  Returns (..., N) in `out_dtype` (default: x.dtype,
    float32 for other inputs)."""
    return _dense_linear("block128", x, w_q, w_scales, bias, out_dtype)


# ---- per-row dynamic quantisation: one scale per row - per token for activations, per output channel for weights (include/fp8mi.h) ----

def fp8_quantize_rowwise(x: torch.Tensor, out_format: int = _l.FMT_E4M3, encode_mode: int | None = None, return_amax: bool = False):
    """Float -> FP8 with one amax scale per row of the last dimension, in one launch on the device (no host read-back):
    fp8_quantize (out_format FMT_E4M3, the module's ENCODE_MODE unless `encode_mode` is given) or fp8_quantize_e5m2 (FMT_E5M2, OCP
    round-to-nearest-even only) applied to every row on its own.

    x: (..., K) float32 / float16 / bfloat16.  Returns (q, inv_scale): q of x's shape - uint8 e4m3fn bytes, or a float8_e5m2 tensor -
    and inv_scale float32 of shape (*x.shape[:-1], 1): the (M, 1) scale_a torch._scaled_mm / fp8_scaled_mm take for activations; a
    weight's goes in as inv_scale.t().  return_amax: also the rows' max|x|, float32 of the same shape, as a third value."""
    assert out_format in (_l.FMT_E4M3, _l.FMT_E5M2), f"unknown out_format {out_format!r}"
    if encode_mode is None:
        encode_mode = ENCODE_MODE if out_format == _l.FMT_E4M3 else _l.ENC_RNE
    x = _float_source(x)
    assert x.dim() >= 1, "per-row quantisation takes a (..., K) tensor"
    lead = tuple(x.shape[:-1])
    x2, rows, cols, ld_in = _rows_view(x)
    dev = x2.device
    q = torch.empty((rows, cols), dtype=torch.uint8, device=dev)
    inv = torch.empty((rows,), dtype=torch.float32, device=dev)
    amax = torch.empty((rows,), dtype=torch.float32, device=dev) if return_amax else None
    _call("fp8mi_quantize_rowwise", dev, x2.data_ptr(), _DTYPE_CODE[x2.dtype], rows, cols, ld_in, q.data_ptr(), max(cols, 1), inv.data_ptr(),
          amax.data_ptr() if return_amax else None, out_format, encode_mode)
    q = q.reshape(*lead, cols)
    if out_format == _l.FMT_E5M2:
        q = q.view(_E5M2)
    if return_amax:
        return q, inv.reshape(*lead, 1), amax.reshape(*lead, 1)
    return q, inv.reshape(*lead, 1)


def fp8_dequantize_rowwise(q: torch.Tensor, scales: torch.Tensor, out_dtype: torch.dtype = torch.float32, in_format: int | None = None) -> torch.Tensor:
    """(..., K) FP8 bytes (uint8 / float8_e4m3fn: e4m3, float8_e5m2: e5m2, or `in_format` for raw bytes) and one float32 scale per row
    (any shape with that many elements, e.g. fp8_quantize_rowwise's (..., 1)) -> dec(q) * scale as out_dtype: OCP decode (NaN bytes
    give NaN), the product in fp32 rounded once, then to out_dtype."""
    fmt = _operand_format(q, in_format, "q")
    assert q.dim() >= 1
    q = _to_device(q)
    if q.dtype != torch.uint8:
        q = q.view(torch.uint8)
    shape = tuple(q.shape)
    q2, rows, cols, ld_in = _rows_view(q)
    dev = q2.device
    s = scales
    if not (s.dtype is torch.float32 and s.device == dev and s.is_contiguous()):
        s = _TO(s, device=dev, dtype=torch.float32).reshape(-1).contiguous()
    assert s.numel() == rows, f"scales has {s.numel()} elements; expected one per row ({rows})"
    out_code = _out_code(out_dtype)
    out = torch.empty(shape, dtype=out_dtype, device=dev)
    _call("fp8mi_dequant_rowwise", dev, q2.data_ptr(), rows, cols, ld_in, s.data_ptr(), fmt, out.data_ptr(), out_code)
    return out


def fp8_linear_rowwise(x: torch.Tensor, weight_u8: torch.Tensor, weight_scale: torch.Tensor, bias: torch.Tensor | None = None,
                       out_dtype: torch.dtype | None = None, weight_format: int | None = None) -> torch.Tensor:
    """y = x @ dequant(W).T + bias with dynamic per-token activation quantisation: fp8_linear with the per-row quantiser - ONE quantise
    launch (fp8_quantize_rowwise, e4m3), then fp8_scaled_mm with a scale_a of M elements and the fused bias / cast epilogue.

    x: (..., K) float32 / float16 / bfloat16;  weight_u8: (N, K) e4m3fn bytes, or e5m2 as in fp8_linear;  weight_scale: [1], or [N]
    for a weight quantised per output channel (fp8_quantize_rowwise(W)).  Returns (..., N) in `out_dtype` (default: x.dtype, float32
    for other inputs)."""
    return _dense_linear("row", x, weight_u8, weight_scale, bias, out_dtype, weight_format)


# ---- fused activation (+ gate product) + quantisation, and the MLPs that stay in FP8 between their two GEMMs (include/fp8mi.h) ----

_ACT_CODE = {"none": _l.ACT_NONE, "silu": _l.ACT_SILU, "gelu_tanh": _l.ACT_GELU_TANH, "gelu_erf": _l.ACT_GELU_ERF}
# The ONE place for the fused producers' scale= (fp8_act_quantize's docstring has the outputs): this table and the three functions below it.
# scale= -> (scale, an MX operand?, one float32 scale per 128 columns?, the suffix of the entry points, the scale_mode / mx_format they take)
_SCALES = {"row": ("row", False, False, "", _l.QSCALE_ROW), "block128": ("block128", False, True, "", _l.QSCALE_GROUP128),
           "mxfp8": ("mxfp8", True, False, "_mx", _l.MX_FP8), "mxfp4": ("mxfp4", True, False, "_mx", _l.MX_FP4)}


def _scale_recipe(scale, out_format=_l.FMT_E4M3, encode_mode=None, return_amax=False):
    """The keywords that go with scale=, validated -> (*_SCALES[scale], out_format, encode_mode with its default filled in)"""
    row = _SCALES.get(scale)
    assert row is not None, f"unknown scale {scale!r}; expected 'row', 'block128', 'mxfp8' or 'mxfp4'"
    if row[1]:
        assert out_format == _l.FMT_E4M3, f"scale={scale!r} fixes the element format: out_format must stay at its default"
        assert encode_mode is None, f"scale={scale!r} has one rounding (the MX recipe's): encode_mode must stay at its default"
        assert not return_amax, f"scale={scale!r} has no per-row amax"
    assert out_format in (_l.FMT_E4M3, _l.FMT_E5M2), f"unknown out_format {out_format!r}"
    assert not (row[2] and return_amax), "scale='block128' has no per-row amax"
    if encode_mode is None:
        encode_mode = _l.ENC_RNE if (row[2] or out_format == _l.FMT_E5M2) else ENCODE_MODE
    return (*row, out_format, encode_mode)


def _scale_outputs(recipe, rows: int, cols: int, dev, amax=(), behind_q=()):
    """-> (the entry point's arguments from q on, q, scales).  The arguments: q, `behind_q` (the scatter forms' rows_out), its leading dimension,
    the scales and their strides, `amax` (a one-tuple: an e4m3 form's pointer, where the entry point has one), the modes.  float32 scales: one per row, or per 128 columns; MX: E8M0 bytes in a (rows,
    round_up(cols / 32, 4)) allocation, which the GEMMs read in place (mxfp8_scale_ld) and whose pad bytes the kernel sets to 0x7F"""
    scale, mx, group, _suffix, kind, out_format, encode_mode = recipe
    if mx:
        assert cols % 32 == 0, f"{cols} columns: {scale} needs a multiple of 32"
        width, ns = (cols // 2 if scale == "mxfp4" else cols), (cols // 32 + 3) // 4 * 4
        q = torch.empty((rows, width), dtype=torch.uint8, device=dev)
        sc = torch.empty((rows, ns), dtype=torch.uint8, device=dev)
        return (q.data_ptr(), *behind_q, max(width, 1), sc.data_ptr(), max(ns, 1), kind), q, sc
    ns = (cols + 127) // 128 if group else 1
    q = torch.empty((rows, cols), dtype=torch.uint8, device=dev)
    sc = torch.empty((rows, ns), dtype=torch.float32, device=dev)
    return (q.data_ptr(), *behind_q, max(cols, 1), sc.data_ptr(), max(ns, 1), 1, *amax, kind, out_format, encode_mode), q, sc


def _scale_results(recipe, q, sc, lead=None, cols=0):
    """-> (q, scales): fp8 bytes (float8_e5m2 for that out_format, float4_e2m1fn_x2 pairs for "mxfp4") and their scales - back in the input's
    leading dimensions `lead`, an MX pair's scales without the pad columns and as float8_e8m0fnu; lead None: the 2-D allocations as they are"""
    if recipe[0] == "mxfp4" and _FP4X2 is not None:
        q = q.view(_FP4X2)
    elif recipe[5] == _l.FMT_E5M2:
        q = q.view(_E5M2)
    if lead is None:
        return q, sc
    if recipe[1]:
        sc = sc[:, :cols // 32]
        if _E8M0 is not None:
            sc = sc.view(_E8M0)
    return q.reshape(*lead, q.shape[-1]), sc.reshape(*lead, sc.shape[-1])


def fp8_act_quantize(x: torch.Tensor, act: str = "none", gated: bool = False, scale: str = "row", out_format: int = _l.FMT_E4M3,
                     encode_mode: int | None = None, return_amax: bool = False):
    """y = act(x) - or act(gate) * up for x = [gate | up] along the last dimension (gated=True, h.chunk(2, -1)) - evaluated in fp32 and
    quantised to FP8 in ONE launch: what fp8_quantize_rowwise (scale="row") or fp8_quantize_blockwise(., 1) (scale="block128") would
    give for y, without y ever reaching memory.

    x: (..., C), or (..., 2C) when gated, float32 / float16 / bfloat16; a 2-D column-slice view is read in place through its row stride.
    act: "none" | "silu" | "gelu_tanh" | "gelu_erf".  Returns (q, scales):
      scale="row":      q (..., C) uint8 e4m3fn bytes (the module's ENCODE_MODE unless `encode_mode` is given) or float8_e5m2 (out_format
                        FMT_E5M2, OCP rounding only), scales float32 (..., 1): the inverse scales, the scale_a of fp8_scaled_mm /
                        torch._scaled_mm; return_amax adds the rows' max|y| as a third value;
      scale="block128": q (..., C) uint8 e4m3fn bytes (OCP rounding), scales float32 (..., ceil(C / 128)) row-major: the scale_a of
                        fp8_scaled_mm_blockwise(block_a=1);
      scale="mxfp8":    q (..., C) uint8 e4m3fn bytes, scales float8_e8m0fnu (..., C / 32): what fp8_quantize_mxfp8 gives for y, the
                        operand of fp8_scaled_mm_mxfp8;  C % 32 == 0;
      scale="mxfp4":    q (..., C / 2) float4_e2m1fn_x2, scales as for "mxfp8": what fp8_quantize_mxfp4 gives for y.
    The MX scales are a view of a (rows, round_up(C / 32, 4)) allocation whose pad bytes are 2^0, so the GEMMs take them in place;
    out_format, encode_mode and return_amax stay at their defaults there."""
    assert act in _ACT_CODE, f"unknown act {act!r}; expected one of {sorted(_ACT_CODE)}"
    recipe = _scale_recipe(scale, out_format, encode_mode, return_amax)
    assert x.dim() >= 1, "takes a (..., C) tensor"
    assert not gated or x.shape[-1] % 2 == 0, f"gated: the last dimension holds [gate | up] and must be even, not {x.shape[-1]}"
    x = _float_source(x)
    lead = tuple(x.shape[:-1])
    x2, rows, width, ld_in = _rows_view(x)
    cols, dev = (width // 2 if gated else width), x2.device
    amax = torch.empty((rows,), dtype=torch.float32, device=dev) if return_amax else None
    args, q, sc = _scale_outputs(recipe, rows, cols, dev, (amax.data_ptr() if return_amax else None,))
    _call("fp8mi_act_quantize" + recipe[3], dev, x2.data_ptr(), _DTYPE_CODE[x2.dtype], rows, cols, ld_in, _ACT_CODE[act] | (_l.ACT_GATED if gated else 0),
          *args)
    q, sc = _scale_results(recipe, q, sc, lead, cols)
    return (q, sc, amax.reshape(*lead, 1)) if return_amax else (q, sc)


# ---- the dense layer ops on their six recipes: one table, three bodies (the MoE layer's are _MOE_RECIPES and the bodies below it) ----

def _act_quantizer(scale: str):
    return lambda x: fp8_act_quantize(x, "none", False, scale)


# One row per recipe.  quantize: how fp8_linear* quantises x; mlp_quantize: how fp8_mlp_* does, and w1_name what its assertions call w1; scale:
# the scale= of the fused producers in the MLP and the norm-linear; mm: the GEMM, and kw its fixed keywords; per_byte: elements per WEIGHT
# byte; e5m2: the weight may be e5m2 (its format goes in as b_format); bytes_checked: whether (the linear, the MLP and the norm-linear) assert a
# one-byte weight themselves or leave that to the GEMM.  quantize and mm are NAMES, looked up in the module at every call as the hand-written
# bodies did (tests/test_gpu_grouped.py forces a tile by replacing fp8_scaled_mm).  The differences between the rows are launch choices with
# measured reasons: the linears quantise with the stand-alone quantisers (fp8_quantize_blockwise at its block_rows = 1),
# the MLPs with the streaming kernel - but for the per-row MLP, whose first layer is fp8_linear_rowwise as it always has been ("weight").
# "tensor" has no fused producer.  mxw4a8: MXFP8 activations against weights of two e2m1 per byte.
_Dense = collections.namedtuple("_Dense", "quantize mlp_quantize w1_name scale mm kw per_byte e5m2 bytes_checked")
_DENSE_RECIPES = {
    "tensor": _Dense("fp8_quantize", None, None, None, "fp8_scaled_mm", {}, 1, True, (False, False)),
    "row": _Dense("fp8_quantize_rowwise", lambda x: fp8_quantize_rowwise(x), "weight", "row", "fp8_scaled_mm", {}, 1, True, (False, False)),
    "block128": _Dense("fp8_quantize_blockwise", _act_quantizer("block128"), "w1", "block128", "fp8_scaled_mm_blockwise",
                       dict(block_a=1, block_b=128), 1, False, (True, True)),
    "mxfp8": _Dense("fp8_quantize_mxfp8", _act_quantizer("mxfp8"), "w1", "mxfp8", "fp8_scaled_mm_mxfp8", {}, 1, False, (True, False)),
    "mxfp4": _Dense("fp8_quantize_mxfp4", _act_quantizer("mxfp4"), "w1", "mxfp4", "fp8_scaled_mm_mxfp4", {}, 2, False, (False, False)),
    "mxw4a8": _Dense("fp8_quantize_mxfp8", _act_quantizer("mxfp8"), "w1", "mxfp8", "fp8_scaled_mm_mxw4a8", {}, 2, False, (False, False)),
}
_B_FORMAT = ({"b_format": _l.FMT_E4M3}, {"b_format": _l.FMT_E5M2})   # (indexed by the format's code)
_module = globals()   # where the rows' names are looked up


def _dense_weight(r, w, what: str, bytes_checked: bool, given=None):
    """The check of an (N, K) weight -> (K, the GEMM's keywords for it)"""
    kw = _B_FORMAT[_operand_format(w, given, what)] if r.e5m2 else r.kw
    assert w.dim() == 2 and (not bytes_checked or w.element_size() == 1)
    return r.per_byte * w.shape[1], kw


def _dense_layer(r, quantize, what, bytes_checked, x, w, w_scales, bias, out_dtype, weight_format=None):
    """(rows, N) = `quantize`(x) against the weight, which the assertions call `what`; out_dtype None: x's (float32 for other inputs)"""
    K, kw = _dense_weight(r, w, what, bytes_checked, weight_format)
    out_dtype = _linear_out_dtype(x, K, out_dtype, what)
    xq, xs = quantize(_to_device(x).reshape(-1, K))
    return _module[r.mm](xq, w, xs, w_scales, bias=bias, out_dtype=out_dtype, **kw)


def _dense_linear(recipe, x, w, w_scales, bias, out_dtype, weight_format=None):
    r = _DENSE_RECIPES[recipe]
    return _like_rows_of(x, _dense_layer(r, _module[r.quantize], "weight", r.bytes_checked[0], x, w, w_scales, bias, out_dtype, weight_format))


def _dense_mlp(recipe, x, w1, w1_scales, w2, w2_scales, act, gated, bias1, bias2, out_dtype):
    r = _DENSE_RECIPES[recipe]
    assert w2.dim() == 2 and (not r.bytes_checked[1] or w2.element_size() == 1)
    h = _dense_layer(r, r.mlp_quantize, r.w1_name, r.bytes_checked[1], x, w1, w1_scales, bias1, None)
    H = h.shape[-1] // 2 if gated else h.shape[-1]
    K2 = r.per_byte * w2.shape[1]
    assert K2 == H, f"w2 expects {K2} hidden features; the first layer gives {H}"
    hq, hs = fp8_act_quantize(h, act, gated, r.scale)
    kw = _B_FORMAT[_operand_format(w2, None, "w2")] if r.e5m2 else r.kw   # (an e5m2-capable recipe looks at w2's type only here, as it always has)
    return _like_rows_of(x, _module[r.mm](hq, w2, hs, w2_scales, bias=bias2, out_dtype=h.dtype if out_dtype is None else out_dtype, **kw))


def _dense_norm_linear(recipe, x, w, w_scales, norm, weight, norm_bias, eps, residual, mod_scale, mod_shift, bias, out_dtype):
    r = _DENSE_RECIPES[recipe]
    K, kw = _dense_weight(r, w, "w", r.bytes_checked[1])
    out_dtype = _linear_out_dtype(x, K, out_dtype)
    got = fp8_norm_quantize(x, norm, weight, norm_bias, eps, residual, mod_scale, mod_shift, r.scale)
    y = _module[r.mm](got[0].reshape(-1, got[0].shape[-1]), w, got[1].reshape(-1, got[1].shape[-1]), w_scales, bias=bias, out_dtype=out_dtype, **kw)
    return (_like_rows_of(x, y), got[2]) if residual is not None else _like_rows_of(x, y)


def fp8_mlp_rowwise(x: torch.Tensor, w1: torch.Tensor, w1_scale: torch.Tensor, w2: torch.Tensor, w2_scale: torch.Tensor, act: str = "silu",
                    gated: bool = True, bias1: torch.Tensor | None = None, bias2: torch.Tensor | None = None,
                    out_dtype: torch.dtype | None = None) -> torch.Tensor:
    """An MLP that stays in FP8 between its two GEMMs, per-row recipe:  h = fp8_linear_rowwise(x, w1, w1_scale, bias1), then ONE launch
    for act (and the gate product) and the per-row quantisation of the result (fp8_act_quantize), then fp8_scaled_mm against w2.

    x: (..., K);  w1: (H, K) - (2H, K) when gated, rows [gate | up] - e4m3fn bytes (or e5m2, as fp8_linear_rowwise);  w2: (N, H);  the
    weight scales [1] or one per output channel.  h has x's dtype (float32 for other inputs).  Returns (..., N) in `out_dtype` (default
    h's dtype)."""
    return _dense_mlp("row", x, w1, w1_scale, w2, w2_scale, act, gated, bias1, bias2, out_dtype)


def fp8_mlp_blockwise(x: torch.Tensor, w1_q: torch.Tensor, w1_scales: torch.Tensor, w2_q: torch.Tensor, w2_scales: torch.Tensor, act: str = "silu",
                      gated: bool = True, bias1: torch.Tensor | None = None, bias2: torch.Tensor | None = None,
                      out_dtype: torch.dtype | None = None) -> torch.Tensor:
    """fp8_mlp_rowwise on the blockwise (DeepSeek) recipe: 1x128 activation scales against 128x128 weight scales in both GEMMs.  x itself
    is quantised by the streaming kernel (act="none", scale="block128": the bytes and scales of fp8_quantize_blockwise(x, 1)); the
    hidden activations by the same kernel with `act` (and the gate product).

    x: (..., K);  w1_q: (H, K) - (2H, K) when gated - e4m3fn bytes with (ceil(rows / 128), ceil(K / 128)) scales;  w2_q: (N, H)."""
    return _dense_mlp("block128", x, w1_q, w1_scales, w2_q, w2_scales, act, gated, bias1, bias2, out_dtype)


# ---- grouped (mixture-of-experts) GEMM: tokens sorted by expert, each run of rows against its own expert's weights (include/fp8mi.h) ----

# the ring tiles that have a grouped form (fp8mi_scaled_mm_grouped / _grouped_blockwise); AUTO too.  No GENERIC, no split-K.
GROUPED_KERNELS = MXFP8_KERNELS


def _grouped_operands(A: torch.Tensor, B: torch.Tensor, offs: torch.Tensor):
    """-> (A, B, offs, M_total, N, K, G, lda, ldb, stride_b, dev): A (M_total, K) and B (G, N, K) e4m3fn bytes whose rows are dense in K (padded
    row and expert strides are read in place, anything else is copied); offs int32[G] cumulative row ends ON THE DEVICE - it is never read here."""
    assert A.dim() == 2 and B.dim() == 3 and A.element_size() == 1 and B.element_size() == 1, "A is (M_total, K) and B (G, N, K), one byte per element"
    assert _operand_format(A, None, "A") == _l.FMT_E4M3 and _operand_format(B, None, "B") == _l.FMT_E4M3, "the grouped forms are e4m3 only"
    M, K = A.shape
    G, N, K2 = B.shape
    assert K2 == K and G >= 1, f"B is {tuple(B.shape)}; expected (G >= 1, N, {K})"
    A = _to_device(A)
    B = _to_device(B)
    dev = A.device
    assert B.device == dev, "A and B must be on the same device"
    A, lda = _operand_rows(A, M, K)
    if not (K == 0 or N == 0 or (B.stride(2) == 1 and B.stride(1) >= K and (G == 1 or B.stride(0) >= (N - 1) * B.stride(1) + K))):
        B = B.contiguous()
    ldb = max(B.stride(1), K) if N > 1 else max(K, 1)
    stride_b = B.stride(0) if G > 1 else max((N - 1) * ldb + K, 0)
    assert isinstance(offs, torch.Tensor) and offs.numel() == G, f"offs needs one cumulative row end per group ({G})"
    if not (offs.dtype is torch.int32 and offs.device == dev and offs.is_contiguous()):
        offs = _TO(offs, device=dev, dtype=torch.int32).contiguous()
    return A, B, offs, M, N, K, G, lda, ldb, stride_b, dev


def _grouped_bias(bias, G: int, N: int, dev):
    if bias is None:
        return None, _l.F32, None
    if bias.device != dev:
        bias = _TO(bias, device=dev)
    if bias.dtype not in _DTYPE_CODE:
        bias = _TO(bias, torch.float32)
    assert bias.numel() == G * N, f"bias has {bias.numel()} elements; expected one row of {N} per expert ({G})"
    bias = bias.contiguous()
    return bias.data_ptr(), _DTYPE_CODE[bias.dtype], bias


def _launch_gemm_grouped(entry: str, operands: tuple, K: int, scales: tuple, modes: tuple, bias, scale_result, out_dtype, out, tail: tuple):
    """_launch_gemm's counterpart for the grouped entry points, behind a function's own scale preparation: the output, the no-op, the bias,
    the ONE ctypes call, the check.  operands: _grouped_operands' result; K: the depth the entry point counts (MXFP4: elements);
    scales: the arguments between C and bias; modes: those between ldc and out_dtype; tail: those between bias_dtype and the stream."""
    A, B, offs, M, N, _k, G, lda, ldb, stride_b, dev = operands
    C, out_code, ldc = _output(out, out_dtype, M, N, dev)
    if M == 0 or N == 0:
        return C
    bias_ptr, bias_code, _keep_bias = _grouped_bias(bias, G, N, dev)
    _unused, _code, sr_ptr, _keep = _epilogue_args(None, scale_result, False, M, N, dev)
    with _on_device(dev):
        rc = getattr(_l.load(), entry)(A.data_ptr(), B.data_ptr(), C.data_ptr(), *scales, bias_ptr, sr_ptr, offs.data_ptr(), G, M, N, K, lda, ldb,
                                       stride_b, ldc, *modes, out_code, bias_code, *tail, _stream(dev))
    if rc:
        _l.check(rc, entry)
    return C


def fp8_scaled_mm_grouped(A: torch.Tensor, B: torch.Tensor, scale_a: torch.Tensor, scale_b: torch.Tensor, offs: torch.Tensor,
                          *, bias: torch.Tensor | None = None, scale_result: torch.Tensor | None = None,
                          out_dtype: torch.dtype | None = None, nan_mode: int | None = None, kernel: int = _l.KERNEL_AUTO,
                          out: torch.Tensor | None = None) -> torch.Tensor:
    """Grouped FP8 matrix multiplication in ONE launch: rows [offs[g-1], offs[g]) of A against expert g's B[g] (include/fp8mi.h,
    fp8mi_scaled_mm_grouped).

    A: (M_total, K) e4m3fn bytes, tokens sorted by expert;  B: (G, N, K);  offs: int32[G] cumulative row ends on the device (never read by
    the host: no sync, capturable into a HIP graph);  scale_a: [1] or [M_total];  scale_b: [G] (one per expert) or [G, N];  bias: None or [G, N].
    Returns (M_total, N) float32 (or `out_dtype`); rows that no group owns are NOT written (a new tensor holds arbitrary values there; pass
    `out` to keep yours).  A group's rows equal fp8_scaled_mm on them with the same tile and split_k=1, bit for bit.
    kernel: AUTO or one of GROUPED_KERNELS."""
    ops = _a, _b, _offs, M, N, K, G, _lda, _ldb, _stride_b, dev = _grouped_operands(A, B, offs)
    sa, sa_mode = _scale_arg(scale_a, dev, M, "scale_a")
    sb = scale_b
    if not (sb.dtype is torch.float32 and sb.device == dev and sb.is_contiguous()):
        sb = _TO(sb, device=dev, dtype=torch.float32).contiguous()
    assert sb.numel() in (G, G * N), f"scale_b has {sb.numel()} elements; expected {G} (one per expert) or {G * N}"
    sb_mode = _l.SCALE_TENSOR if sb.numel() == G else _l.SCALE_ROW
    return _launch_gemm_grouped("fp8mi_scaled_mm_grouped", ops, K, (sa.data_ptr(), sb.data_ptr()), (sa_mode, sb_mode), bias, scale_result, out_dtype, out,
                                (NAN_MODE if nan_mode is None else nan_mode, kernel))


def fp8_scaled_mm_grouped_blockwise(A: torch.Tensor, B: torch.Tensor, scale_a: torch.Tensor, scale_b: torch.Tensor, offs: torch.Tensor,
                                    *, block_b: int = 128, bias: torch.Tensor | None = None, scale_result: torch.Tensor | None = None,
                                    out_dtype: torch.dtype | None = None, nan_mode: int | None = None, kernel: int = _l.KERNEL_AUTO,
                                    out: torch.Tensor | None = None) -> torch.Tensor:
    """fp8_scaled_mm_grouped on the blockwise (DeepSeek) recipe: scale_a (M_total, ceil(K/128)) float32, one per 128 k of every row (block_a is
    always 1: group starts are not 128-aligned);  scale_b (G, ceil(N / block_b), ceil(K/128)) float32, any strides, block_b 1 or 128.  A group's
    rows equal fp8_scaled_mm_blockwise on them with the same tile and split_k=1, bit for bit."""
    ops = _a, _b, _offs, M, N, K, G, _lda, _ldb, _stride_b, dev = _grouped_operands(A, B, offs)
    sa, sa_sr, sa_sk = _bw_scales(scale_a, M, K, 1, dev, "scale_a")
    assert block_b in (1, 128), f"scale_b: block must be 1 or 128, not {block_b}"
    shape_b = (G, (N + block_b - 1) // block_b, (K + 127) // 128)
    assert scale_b.dim() == 3 and tuple(scale_b.shape) == shape_b, f"scale_b: {tuple(scale_b.shape)} scales; expected {shape_b}"
    sb = scale_b
    if not (sb.dtype is torch.float32 and sb.device == dev):
        sb = _TO(sb, device=dev, dtype=torch.float32)
    return _launch_gemm_grouped("fp8mi_scaled_mm_grouped_blockwise", ops, K,
                                (sa.data_ptr(), sa_sr, sa_sk, 1, sb.data_ptr(), sb.stride(1), sb.stride(2), sb.stride(0), block_b), (), bias,
                                scale_result, out_dtype, out, (NAN_MODE if nan_mode is None else nan_mode, kernel))


def _grouped_mx_scales_b(scale: torch.Tensor, G: int, N: int, K: int, dev):
    """-> (uint8 tensor on dev that holds the experts' (G, N, K/32) E8M0 scales, ld_sb, stride_sb).  A layout the kernels read - unit
    stride along K, row and expert strides multiples of 4, a 4-byte aligned base - is taken in place; anything else is copied once into
    (G, N, round_up(K/32, 4)) with pad bytes 2^0."""
    s = _e8m0_bytes(scale)
    if s.device != dev:
        s = _TO(s, device=dev)
    nb = K // 32
    assert s.dim() == 3 and s.shape[0] == G and s.shape[1] == N and s.shape[2] >= nb, \
        f"scale_b: {tuple(scale.shape)} E8M0 scales; expected ({G}, {N}, {nb})"
    ok = (nb == 0 or N == 0 or ((s.stride(2) == 1 or s.shape[2] == 1) and (N == 1 or (s.stride(1) >= nb and s.stride(1) % 4 == 0)) and
                               (G == 1 or (s.stride(0) % 4 == 0 and s.stride(0) >= (N - 1) * (s.stride(1) if N > 1 else 0) + nb)) and
                               s.data_ptr() % 4 == 0))
    if not ok:
        buf = torch.full((G, N, (nb + 3) // 4 * 4), 0x7F, dtype=torch.uint8, device=dev)
        buf[:, :, :nb].copy_(s[:, :, :nb])
        s = buf
    ld = max(s.stride(1) if N > 1 else (nb + 3) // 4 * 4, 4)   # (a single row or expert has no stride of its own: the smallest legal one)
    stride = s.stride(0) if G > 1 else ((N - 1) * ld + nb + 3) // 4 * 4
    return s, ld, stride


def _grouped_operands_mxw4a8(A: torch.Tensor, B: torch.Tensor, offs: torch.Tensor):
    """_grouped_operands for A (M_total, K) e4m3fn bytes against B (G, N, K/2) e2m1 pairs: the same tuple, K in elements, strides in bytes"""
    assert A.dim() == 2 and B.dim() == 3 and A.element_size() == 1, "A is (M_total, K) bytes and B (G, N, K/2) e2m1 pairs"
    assert _operand_format(A, None, "A") == _l.FMT_E4M3, "the activations are e4m3"
    B = _fp4_bytes(B)
    M, K = A.shape
    G, N, Kb = B.shape
    assert 2 * Kb == K and G >= 1, f"B is {tuple(B.shape)}; expected (G >= 1, N, {K // 2}) for K={K}"
    A = _to_device(A)
    B = _to_device(B)
    dev = A.device
    assert B.device == dev, "A and B must be on the same device"
    A, lda = _operand_rows(A, M, K)
    if not (Kb == 0 or N == 0 or (B.stride(2) == 1 and B.stride(1) >= Kb and (G == 1 or B.stride(0) >= (N - 1) * B.stride(1) + Kb))):
        B = B.contiguous()
    ldb = max(B.stride(1), Kb) if N > 1 else max(Kb, 1)
    stride_b = B.stride(0) if G > 1 else max((N - 1) * ldb + Kb, 0)
    assert isinstance(offs, torch.Tensor) and offs.numel() == G, f"offs needs one cumulative row end per group ({G})"
    if not (offs.dtype is torch.int32 and offs.device == dev and offs.is_contiguous()):
        offs = _TO(offs, device=dev, dtype=torch.int32).contiguous()
    return A, B, offs, M, N, K, G, lda, ldb, stride_b, dev


def _scaled_mm_grouped_mx(fp4, A, B, scale_a, scale_b, offs, bias, scale_result, out_dtype, nan_mode, kernel, out):
    """The two MX forms, on the operands' bytes: A (M_total, Kb) and B (G, N, Kb), Kb = K (MXFP8) or K / 2 (MXFP4), the strides in bytes."""
    ops = _a, _b, _offs, M, N, Kb, G, _lda, _ldb, _stride_b, dev = _grouped_operands(_fp4_bytes(A), _fp4_bytes(B), offs) if fp4 else \
        _grouped_operands(A, B, offs)
    K = 2 * Kb if fp4 else Kb
    assert K % 32 == 0, f"K={K}: the MX recipes need a multiple of the 32-element scale block"
    sa, ld_sa = _mx_scales(scale_a, M, K, dev, "scale_a")
    sb, ld_sb, stride_sb = _grouped_mx_scales_b(scale_b, G, N, K, dev)
    return _launch_gemm_grouped("fp8mi_scaled_mm_grouped_mxfp4" if fp4 else "fp8mi_scaled_mm_grouped_mxfp8", ops, K,
                                (sa.data_ptr(), ld_sa, sb.data_ptr(), ld_sb, stride_sb), (), bias, scale_result, out_dtype, out,
                                (kernel,) if fp4 else (NAN_MODE if nan_mode is None else nan_mode, kernel))   # (the MXFP4 entry has no nan_mode)


def fp8_scaled_mm_grouped_mxfp8(A: torch.Tensor, B: torch.Tensor, scale_a: torch.Tensor, scale_b: torch.Tensor, offs: torch.Tensor,
                                *, bias: torch.Tensor | None = None, scale_result: torch.Tensor | None = None,
                                out_dtype: torch.dtype | None = None, nan_mode: int | None = None, kernel: int = _l.KERNEL_AUTO,
                                out: torch.Tensor | None = None) -> torch.Tensor:
    """fp8_scaled_mm_grouped on the MXFP8 recipe, in ONE launch (include/fp8mi.h, fp8mi_scaled_mm_grouped_mxfp8).

    A: (M_total, K) e4m3fn bytes sorted by expert;  B: (G, N, K);  scale_a: (M_total, K/32) E8M0 (float8_e8m0fnu or uint8; the padded
    allocations of fp8_act_quantize / fp8_moe_scatter_quantize are read in place);  scale_b: (G, N, K/32), read in place when its row and
    expert strides are multiples of 4;  offs, bias [G, N], scale_result, out and the unwritten rows as in fp8_scaled_mm_grouped.  A group's
    rows equal fp8_scaled_mm_mxfp8 on them with the same tile and split_k=1, bit for bit.  kernel: AUTO or one of GROUPED_KERNELS."""
    return _scaled_mm_grouped_mx(False, A, B, scale_a, scale_b, offs, bias, scale_result, out_dtype, nan_mode, kernel, out)


def fp8_scaled_mm_grouped_mxfp4(A: torch.Tensor, B: torch.Tensor, scale_a: torch.Tensor, scale_b: torch.Tensor, offs: torch.Tensor,
                                *, bias: torch.Tensor | None = None, scale_result: torch.Tensor | None = None,
                                out_dtype: torch.dtype | None = None, kernel: int = _l.KERNEL_AUTO, out: torch.Tensor | None = None) -> torch.Tensor:
    """fp8_scaled_mm_grouped_mxfp8 with e2m1 elements: A (M_total, K/2) and B (G, N, K/2) float4_e2m1fn_x2 (or uint8), two codes per byte;
    the scales count K/32 blocks of ELEMENTS.  A group's rows equal fp8_scaled_mm_mxfp4 on them with the same tile and split_k=1."""
    return _scaled_mm_grouped_mx(True, A, B, scale_a, scale_b, offs, bias, scale_result, out_dtype, None, kernel, out)


def fp8_scaled_mm_grouped_mxw4a8(A: torch.Tensor, B: torch.Tensor, scale_a: torch.Tensor, scale_b: torch.Tensor, offs: torch.Tensor,
                                 *, bias: torch.Tensor | None = None, scale_result: torch.Tensor | None = None,
                                 out_dtype: torch.dtype | None = None, nan_mode: int | None = None, kernel: int = _l.KERNEL_AUTO,
                                 out: torch.Tensor | None = None) -> torch.Tensor:
    """fp8_scaled_mm_grouped_mxfp8 against e2m1 weights: A (M_total, K) e4m3fn bytes, B (G, N, K/2) float4_e2m1fn_x2 (or uint8); scales,
    offs, bias, out and the unwritten rows as there.  A group's rows equal fp8_scaled_mm_mxw4a8 on them with the same tile and split_k=1,
    bit for bit, under either nan_mode.  kernel: AUTO or one of GROUPED_KERNELS."""
    ops = _a, _b, _offs, M, N, K, G, _lda, _ldb, _stride_b, dev = _grouped_operands_mxw4a8(A, B, offs)
    assert K % 32 == 0, f"K={K}: the MX recipes need a multiple of the 32-element scale block"
    sa, ld_sa = _mx_scales(scale_a, M, K, dev, "scale_a")
    sb, ld_sb, stride_sb = _grouped_mx_scales_b(scale_b, G, N, K, dev)
    return _launch_gemm_grouped("fp8mi_scaled_mm_grouped_mxw4a8", ops, K, (sa.data_ptr(), ld_sa, sb.data_ptr(), ld_sb, stride_sb), (), bias,
                                scale_result, out_dtype, out, (NAN_MODE if nan_mode is None else nan_mode, kernel))


# ---- MoE routing on the device: expert sort, scatter-quantise, combine (include/fp8mi.h, fp8mi_moe_*) -------------------------------------

# fp8mi_moe_route's workspaces, per (device, stream) like the split-K ones: a list whose LAST element serves new calls.  A call that needs
# more appends a larger one (never while the stream is being captured); the superseded ones stay in the list for the life of the process,
# because a HIP graph captured earlier still holds their pointers and writes through them on every replay.
_route_workspaces: dict = {}


def _route_workspace(dev, stream, need: int):
    key = (dev.index, stream)
    held = _route_workspaces.get(key)
    if held is None or held[-1].numel() < need:
        assert not torch.cuda.is_current_stream_capturing(), \
            "fp8_moe_route: this many assignments need a workspace; call it once at this size before capturing"
        with _workspaces_lock:
            held = _route_workspaces.setdefault(key, [])
            if not held or held[-1].numel() < need:
                held.append(torch.empty(need, dtype=torch.uint8, device=dev))
    return held[-1]


def _row_plan(row_of: torch.Tensor, dev, what: str):
    """-> row_of as the kernels read it: int32 (T, k), contiguous, on `dev`"""
    assert row_of.dim() == 2, f"{what}: row_of is (T, k)"
    if not (row_of.dtype is torch.int32 and row_of.device == dev and row_of.is_contiguous()):
        row_of = _TO(row_of, device=dev, dtype=torch.int32).contiguous()
    return row_of


def fp8_moe_route(topk_ids: torch.Tensor, G: int):
    """The gate's expert ids -> the sorted-row plan of the grouped GEMMs, on the device (a stable sort by expert; the host reads nothing).

    topk_ids: (T, k) int32 or int64 (torch.topk's indices as they are).  An id outside [0, G) drops its assignment - how an
    expert-parallel caller masks other ranks' experts.  Returns (offs, row_of, src_of_row), int32:
      offs (G,)        cumulative row ends, the offs of fp8_scaled_mm_grouped / fp8_moe_*;
      row_of (T, k)    the row of assignment (t, j) among the T k sorted rows; -1 if dropped;
      src_of_row (T k,) the flat assignment index t k + j of every row below offs[-1]; -1 from there on.
    One launch up to MOE_ROUTE_SINGLE_MAX assignments, three beyond.  The three-launch form uses a workspace cached per (device, stream): to
    capture it into a HIP graph, call it once at that size on the capturing stream first (torch's usual side-stream warm-up and
    torch.cuda.graph(g, stream=side)); workspaces are never released, so a captured graph stays valid when a later call needs a larger one."""
    assert topk_ids.dim() == 2, "topk_ids is (T, k)"
    ids = _to_device(topk_ids)
    if ids.dtype not in (torch.int32, torch.int64):
        ids = _TO(ids, torch.int64)
    ids = ids.contiguous()
    dev, n = ids.device, ids.numel()
    row_of = torch.empty(tuple(ids.shape), dtype=torch.int32, device=dev)
    src_of_row = torch.empty((n,), dtype=torch.int32, device=dev)
    if n == 0:
        assert 1 <= G <= 1024, f"G={G}: 1 to 1024 experts"
        return torch.zeros((G,), dtype=torch.int32, device=dev), row_of, src_of_row
    offs = torch.empty((max(G, 0),), dtype=torch.int32, device=dev)
    lib = _l.load()
    with _on_device(dev):
        stream = _stream(dev)
        need = int(lib.fp8mi_moe_route_workspace_bytes(n, G))
        ws = _route_workspace(dev, stream, need) if need > 0 else None
        rc = lib.fp8mi_moe_route(ids.data_ptr(), ids.element_size(), n, G, offs.data_ptr(), row_of.data_ptr(), src_of_row.data_ptr(),
                                 ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0, stream)
    _l.check(rc, "fp8mi_moe_route")
    return offs, row_of, src_of_row


def fp8_moe_scatter_quantize(x: torch.Tensor, row_of: torch.Tensor, scale: str = "row", encode_mode: int | None = None):
    """Quantise every token ONCE and store it to each of its k sorted rows: the quantised operand of the grouped GEMMs in one launch, without
    the (T k, K) 16-bit copy of x an index_select would write.

    x: (T, K) float32 / float16 / bfloat16, K a multiple of 16 up to 16384;  row_of: (T, k) int32 (fp8_moe_route).  Returns (q, scales):
    q (T k, K) uint8 e4m3fn bytes, scales float32 (T k, 1) (scale="row": the inverse scales of fp8_quantize_rowwise, the module's
    ENCODE_MODE unless `encode_mode` is given) or (T k, ceil(K / 128)) (scale="block128": fp8_act_quantize(x, "none", False,
    "block128")'s).  Row r holds token src_of_row[r] // k bit for bit; rows no assignment names are NOT written (arbitrary values).
    scale="mxfp8" / "mxfp4" (K a multiple of 32): q (T k, K) e4m3fn bytes / (T k, K/2) e2m1 pairs and scales uint8 (T k, round_up(K/32, 4)),
    the bytes and E8M0 scales of fp8_quantize_mxfp8 / _mxfp4 of the token, pad bytes 2^0 - the operands of fp8_scaled_mm_grouped_mx*."""
    recipe = _scale_recipe(scale, encode_mode=encode_mode)
    x = _float_source(x)
    assert x.dim() == 2, "x is (T, K)"
    x2, T, cols, ld_in = _rows_view(x)
    dev = x2.device
    row_of = _row_plan(row_of, dev, "fp8_moe_scatter_quantize")
    assert row_of.shape[0] == T, f"row_of has {row_of.shape[0]} rows; x has {T} tokens"
    k = row_of.shape[1]
    args, q, sc = _scale_outputs(recipe, T * k, cols, dev, behind_q=(T * k,))
    _call("fp8mi_moe_scatter_quantize" + recipe[3], dev, x2.data_ptr(), _DTYPE_CODE[x2.dtype], T, cols, ld_in, row_of.data_ptr(), k, *args)
    return _scale_results(recipe, q, sc)


def fp8_moe_combine(y: torch.Tensor, row_of: torch.Tensor, weights: torch.Tensor | None = None, out_dtype: torch.dtype | None = None) -> torch.Tensor:
    """The weighted un-permute: out[t] = sum_j weights[t, j] * y[row_of[t, j]], in float32, the k terms added in order j = 0 .. k-1 with every
    product and every sum rounded on its own (reproducible: a gather, no atomics).  Dropped assignments (row_of -1, or any row outside y)
    are skipped; a token without any gets zeros.

    y: (rows, N) float32 / float16 / bfloat16;  row_of: (T, k) int32;  weights: (T, k) (float32 is read in place) or None for 1.
    Returns (T, N) in `out_dtype` (default: y's)."""
    y = _to_device(y)
    if y.dtype not in _DTYPE_CODE:
        y = _TO(y, torch.float32)
    assert y.dim() == 2, "y is (rows, N)"
    y2, rows, N, ld_y = _rows_view(y)
    dev = y2.device
    row_of = _row_plan(row_of, dev, "fp8_moe_combine")
    T, k = row_of.shape
    if weights is not None:
        assert tuple(weights.shape) == (T, k), f"weights is {tuple(weights.shape)}; row_of is {(T, k)}"
        if not (weights.dtype is torch.float32 and weights.device == dev and weights.is_contiguous()):
            weights = _TO(weights, device=dev, dtype=torch.float32).contiguous()
    out, out_code, ld_out = _output(None, y2.dtype if out_dtype is None else out_dtype, T, N, dev)
    with _on_device(dev):
        rc = _l.load().fp8mi_moe_combine(y2.data_ptr(), _DTYPE_CODE[y2.dtype], rows, N, ld_y, row_of.data_ptr(),
                                         weights.data_ptr() if weights is not None else None, T, k, out.data_ptr(), out_code, ld_out, _stream(dev))
    _l.check(rc, "fp8mi_moe_combine")
    return out


# ---- the MoE layer on the four recipes: quantise x, grouped GEMM, activation + quantise, grouped GEMM (include/fp8mi.h) ----

# recipe -> (how fp8_moe_linear_* quantises x, how fp8_moe_mlp_* does, the grouped GEMM, elements per WEIGHT byte, the activations' scale=
# of fp8_act_quantize between an MLP's two GEMMs and of fp8_moe_scatter_quantize in the forward).  The blockwise linear and MLP quantise x
# with different launches, as they always have.  mxw4a8: MXFP8 activations against weights of two e2m1 per byte.
_MOE_RECIPES = {
    "row": (fp8_quantize_rowwise, fp8_quantize_rowwise, fp8_scaled_mm_grouped, 1, "row"),
    "block128": (lambda x: fp8_quantize_blockwise(x, 1), _act_quantizer("block128"), fp8_scaled_mm_grouped_blockwise, 1, "block128"),
    "mxfp8": (_act_quantizer("mxfp8"), _act_quantizer("mxfp8"), fp8_scaled_mm_grouped_mxfp8, 1, "mxfp8"),
    "mxfp4": (_act_quantizer("mxfp4"), _act_quantizer("mxfp4"), fp8_scaled_mm_grouped_mxfp4, 2, "mxfp4"),
    "mxw4a8": (_act_quantizer("mxfp8"), _act_quantizer("mxfp8"), fp8_scaled_mm_grouped_mxw4a8, 2, "mxfp8"),
}


def _moe_linear(recipe, x, offs, w_q, w_scales, bias, out_dtype, kernel):
    quantize, _mlp_quantize, mm, per_byte, _scale = _MOE_RECIPES[recipe]
    assert w_q.dim() == 3 and x.dim() == 2
    out_dtype = _linear_out_dtype(x, per_byte * w_q.shape[2], out_dtype)
    xq, xs = quantize(_to_device(x))
    return mm(xq, w_q, xs, w_scales, offs, bias=bias, out_dtype=out_dtype, kernel=kernel)


def _moe_mlp_quantised(recipe, xq, xs, h_dtype, offs, w1, w1_scales, w2, w2_scales, act, gated, bias1, bias2, out_dtype, kernel):
    """An MoE MLP from its quantised operand on: the grouped gate_up GEMM, act + the recipe's quantisation in one launch, the grouped down GEMM."""
    mm, per_byte, scale = _MOE_RECIPES[recipe][2:]
    h = mm(xq, w1, xs, w1_scales, offs, bias=bias1, out_dtype=h_dtype, kernel=kernel)
    H = h.shape[-1] // 2 if gated else h.shape[-1]
    assert per_byte * w2.shape[2] == H, f"w2 expects {per_byte * w2.shape[2]} hidden features; the first layer gives {H}"
    hq, hs = fp8_act_quantize(h, act, gated, scale)
    return mm(hq, w2, hs, w2_scales, offs, bias=bias2, out_dtype=h_dtype if out_dtype is None else out_dtype, kernel=kernel)


def _moe_mlp(recipe, x, offs, w1, w1_scales, w2, w2_scales, act, gated, bias1, bias2, out_dtype, kernel, w1_name="w1"):
    _quantize, quantize, _mm, per_byte, _scale = _MOE_RECIPES[recipe]
    assert w1.dim() == 3 and w2.dim() == 3 and x.dim() == 2
    h_dtype = _linear_out_dtype(x, per_byte * w1.shape[2], None, w1_name)
    xq, xs = quantize(_to_device(x))
    return _moe_mlp_quantised(recipe, xq, xs, h_dtype, offs, w1, w1_scales, w2, w2_scales, act, gated, bias1, bias2, out_dtype, kernel)


def _moe_forward(recipe, x, topk_ids, topk_weights, w1, w1_scales, w2, w2_scales, act, gated, bias1, bias2, out_dtype, kernel):
    per_byte, scale = _MOE_RECIPES[recipe][3:]
    assert w1.dim() == 3 and w2.dim() == 3 and x.dim() == 2 and topk_ids.dim() == 2 and topk_ids.shape[0] == x.shape[0]
    h_dtype = _linear_out_dtype(x, per_byte * w1.shape[2], None, "w1")
    if x.shape[0] == 0:   # no tokens: nothing to launch
        return torch.empty((0, w2.shape[1]), dtype=h_dtype if out_dtype is None else out_dtype, device=_to_device(x).device)
    offs, row_of, _src = fp8_moe_route(topk_ids, w1.shape[0])
    xq, xs = fp8_moe_scatter_quantize(x, row_of, scale)
    y = _moe_mlp_quantised(recipe, xq, xs, h_dtype, offs, w1, w1_scales, w2, w2_scales, act, gated, bias1, bias2, None, kernel)
    return fp8_moe_combine(y, row_of, topk_weights, h_dtype if out_dtype is None else out_dtype)


def fp8_moe_linear_rowwise(x: torch.Tensor, offs: torch.Tensor, w_q: torch.Tensor, w_scale: torch.Tensor, bias: torch.Tensor | None = None,
                           out_dtype: torch.dtype | None = None, kernel: int = _l.KERNEL_AUTO) -> torch.Tensor:
    """The experts' linear layers in two launches: fp8_linear_rowwise for every expert at once.  x: (M_total, K) float32 / float16 / bfloat16,
    tokens sorted by expert (fp8_moe_route gives the plan from the gate's ids, fp8_moe_forward_* the whole layer);  offs: int32[G] cumulative row ends on the device;  w_q: (G, N, K)
    e4m3fn bytes;  w_scale: [G] or [G, N];  bias: None or [G, N].  Returns (M_total, N) in `out_dtype` (default: x.dtype); rows no expert
    owns are not written."""
    return _moe_linear("row", x, offs, w_q, w_scale, bias, out_dtype, kernel)


def fp8_moe_linear_blockwise(x: torch.Tensor, offs: torch.Tensor, w_q: torch.Tensor, w_scales: torch.Tensor, bias: torch.Tensor | None = None,
                             out_dtype: torch.dtype | None = None, kernel: int = _l.KERNEL_AUTO) -> torch.Tensor:
    """fp8_moe_linear_rowwise on the blockwise recipe (fp8_linear_blockwise per expert): 1x128 activation scales against the experts'
    128x128 weight scales w_scales (G, ceil(N/128), ceil(K/128))."""
    return _moe_linear("block128", x, offs, w_q, w_scales, bias, out_dtype, kernel)


def fp8_moe_linear_mxfp8(x: torch.Tensor, offs: torch.Tensor, w_q: torch.Tensor, w_scales: torch.Tensor, bias: torch.Tensor | None = None,
                         out_dtype: torch.dtype | None = None, kernel: int = _l.KERNEL_AUTO) -> torch.Tensor:
    """fp8_moe_linear_rowwise on the MXFP8 recipe (fp8_linear_mxfp8 per expert), two launches: the streaming MX quantiser, then the grouped
    GEMM.  w_q: (G, N, K) e4m3fn bytes;  w_scales: (G, N, K/32) E8M0."""
    return _moe_linear("mxfp8", x, offs, w_q, w_scales, bias, out_dtype, kernel)


def fp8_moe_linear_mxfp4(x: torch.Tensor, offs: torch.Tensor, w_q: torch.Tensor, w_scales: torch.Tensor, bias: torch.Tensor | None = None,
                         out_dtype: torch.dtype | None = None, kernel: int = _l.KERNEL_AUTO) -> torch.Tensor:
    """fp8_moe_linear_mxfp8 with e2m1 elements: w_q (G, N, K/2) pairs (fp8_quantize_mxfp4 of every expert's weight)."""
    return _moe_linear("mxfp4", x, offs, w_q, w_scales, bias, out_dtype, kernel)


def fp8_moe_linear_mxw4a8(x: torch.Tensor, offs: torch.Tensor, w_q: torch.Tensor, w_scales: torch.Tensor, bias: torch.Tensor | None = None,
                          out_dtype: torch.dtype | None = None, kernel: int = _l.KERNEL_AUTO) -> torch.Tensor:
    """fp8_moe_linear_mxfp8 against e2m1 weights (fp8_linear_mxw4a8 per expert): x is quantised to MXFP8, w_q (G, N, K/2) is
    fp8_quantize_mxfp4's pairs of every expert's weight."""
    return _moe_linear("mxw4a8", x, offs, w_q, w_scales, bias, out_dtype, kernel)


def fp8_moe_mlp_rowwise(x: torch.Tensor, offs: torch.Tensor, w1: torch.Tensor, w1_scale: torch.Tensor, w2: torch.Tensor, w2_scale: torch.Tensor,
                        act: str = "silu", gated: bool = True, bias1: torch.Tensor | None = None, bias2: torch.Tensor | None = None,
                        out_dtype: torch.dtype | None = None, kernel: int = _l.KERNEL_AUTO) -> torch.Tensor:
    """The experts' MLPs, fp8_mlp_rowwise for every expert at once, in four launches: per-row quantisation of x, the grouped gate_up GEMM, ONE
    launch for act (and the gate product) and the per-row quantisation of the result, the grouped down GEMM.

    x: (M_total, K) sorted by expert;  w1: (G, H, K) - (G, 2H, K) when gated, rows [gate | up];  w2: (G, N, H);  scales [G] or one per output
    channel of every expert;  biases None or [G, .].  Rows no expert owns are not written."""
    return _moe_mlp("row", x, offs, w1, w1_scale, w2, w2_scale, act, gated, bias1, bias2, out_dtype, kernel,
                    w1_name="weight")   # (this one function has always named w1 "weight" when x has another width)


def fp8_moe_mlp_blockwise(x: torch.Tensor, offs: torch.Tensor, w1_q: torch.Tensor, w1_scales: torch.Tensor, w2_q: torch.Tensor, w2_scales: torch.Tensor,
                          act: str = "silu", gated: bool = True, bias1: torch.Tensor | None = None, bias2: torch.Tensor | None = None,
                          out_dtype: torch.dtype | None = None, kernel: int = _l.KERNEL_AUTO) -> torch.Tensor:
    """fp8_moe_mlp_rowwise on the blockwise recipe (fp8_mlp_blockwise per expert): 1x128 activation scales, the experts' 128x128 weight scales."""
    return _moe_mlp("block128", x, offs, w1_q, w1_scales, w2_q, w2_scales, act, gated, bias1, bias2, out_dtype, kernel)


def fp8_moe_mlp_mxfp8(x: torch.Tensor, offs: torch.Tensor, w1_q: torch.Tensor, w1_scales: torch.Tensor, w2_q: torch.Tensor, w2_scales: torch.Tensor,
                      act: str = "silu", gated: bool = True, bias1: torch.Tensor | None = None, bias2: torch.Tensor | None = None,
                      out_dtype: torch.dtype | None = None, kernel: int = _l.KERNEL_AUTO) -> torch.Tensor:
    """fp8_moe_mlp_rowwise on the MXFP8 recipe (fp8_mlp_mxfp8 per expert), four launches: the MX quantiser, the grouped gate_up GEMM, ONE launch
    for act (and the gate product) and the MX quantisation of the result, the grouped down GEMM.  K and H multiples of 32;  w1_q (G, H, K) -
    (G, 2H, K) when gated - with (G, rows, K/32) E8M0 scales;  w2_q (G, N, H)."""
    return _moe_mlp("mxfp8", x, offs, w1_q, w1_scales, w2_q, w2_scales, act, gated, bias1, bias2, out_dtype, kernel)


def fp8_moe_mlp_mxfp4(x: torch.Tensor, offs: torch.Tensor, w1_q: torch.Tensor, w1_scales: torch.Tensor, w2_q: torch.Tensor, w2_scales: torch.Tensor,
                      act: str = "silu", gated: bool = True, bias1: torch.Tensor | None = None, bias2: torch.Tensor | None = None,
                      out_dtype: torch.dtype | None = None, kernel: int = _l.KERNEL_AUTO) -> torch.Tensor:
    """fp8_moe_mlp_mxfp8 with e2m1 elements: w1_q (G, H, K/2) - (G, 2H, K/2) when gated - and w2_q (G, N, H/2) are fp8_quantize_mxfp4's pairs."""
    return _moe_mlp("mxfp4", x, offs, w1_q, w1_scales, w2_q, w2_scales, act, gated, bias1, bias2, out_dtype, kernel)


def fp8_moe_mlp_mxw4a8(x: torch.Tensor, offs: torch.Tensor, w1_q: torch.Tensor, w1_scales: torch.Tensor, w2_q: torch.Tensor, w2_scales: torch.Tensor,
                       act: str = "silu", gated: bool = True, bias1: torch.Tensor | None = None, bias2: torch.Tensor | None = None,
                       out_dtype: torch.dtype | None = None, kernel: int = _l.KERNEL_AUTO) -> torch.Tensor:
    """fp8_moe_mlp_mxfp8 against e2m1 weights (fp8_mlp_mxw4a8 per expert), the same four launches: both activations are quantised to MXFP8,
    w1_q (G, H, K/2) - (G, 2H, K/2) when gated - and w2_q (G, N, H/2) are fp8_quantize_mxfp4's pairs."""
    return _moe_mlp("mxw4a8", x, offs, w1_q, w1_scales, w2_q, w2_scales, act, gated, bias1, bias2, out_dtype, kernel)


def fp8_moe_forward_rowwise(x: torch.Tensor, topk_ids: torch.Tensor, topk_weights: torch.Tensor | None, w1: torch.Tensor, w1_scale: torch.Tensor,
                            w2: torch.Tensor, w2_scale: torch.Tensor, act: str = "silu", gated: bool = True, bias1: torch.Tensor | None = None,
                            bias2: torch.Tensor | None = None, out_dtype: torch.dtype | None = None, kernel: int = _l.KERNEL_AUTO) -> torch.Tensor:
    """A whole MoE layer from what the gate gives, per-row recipe: fp8_moe_route -> fp8_moe_scatter_quantize -> the grouped gate_up GEMM ->
    fp8_act_quantize -> the grouped down GEMM -> fp8_moe_combine.  Six launches up to MOE_ROUTE_SINGLE_MAX assignments (eight beyond), all
    over T k rows whatever the routing: nothing is read on the host, and the call captures into a HIP graph that replays on new ids and
    weights.

    x: (T, K);  topk_ids: (T, k) int32 / int64, ids outside [0, G) dropped;  topk_weights: (T, k) or None;  the weights, scales, biases,
    act and gated of fp8_moe_mlp_rowwise.  The experts' outputs have x's dtype (float32 for other inputs); the sum over a token's k
    experts is fp32 (fp8_moe_combine), returned as (T, N) in `out_dtype` (default: that dtype).  Equals fp8_moe_mlp_rowwise on
    x[src_of_row // k] followed by the combine, bit for bit."""
    return _moe_forward("row", x, topk_ids, topk_weights, w1, w1_scale, w2, w2_scale, act, gated, bias1, bias2, out_dtype, kernel)


def fp8_moe_forward_blockwise(x: torch.Tensor, topk_ids: torch.Tensor, topk_weights: torch.Tensor | None, w1_q: torch.Tensor, w1_scales: torch.Tensor,
                              w2_q: torch.Tensor, w2_scales: torch.Tensor, act: str = "silu", gated: bool = True, bias1: torch.Tensor | None = None,
                              bias2: torch.Tensor | None = None, out_dtype: torch.dtype | None = None, kernel: int = _l.KERNEL_AUTO) -> torch.Tensor:
    """fp8_moe_forward_rowwise on the blockwise recipe (fp8_moe_mlp_blockwise between the routing and the combine): 1x128 activation scales,
    the experts' 128x128 weight scales."""
    return _moe_forward("block128", x, topk_ids, topk_weights, w1_q, w1_scales, w2_q, w2_scales, act, gated, bias1, bias2, out_dtype, kernel)


def fp8_moe_forward_mxfp8(x: torch.Tensor, topk_ids: torch.Tensor, topk_weights: torch.Tensor | None, w1_q: torch.Tensor, w1_scales: torch.Tensor,
                          w2_q: torch.Tensor, w2_scales: torch.Tensor, act: str = "silu", gated: bool = True, bias1: torch.Tensor | None = None,
                          bias2: torch.Tensor | None = None, out_dtype: torch.dtype | None = None, kernel: int = _l.KERNEL_AUTO) -> torch.Tensor:
    """fp8_moe_forward_rowwise on the MXFP8 recipe: fp8_moe_route -> fp8_moe_scatter_quantize(scale="mxfp8") -> the grouped MX gate_up GEMM ->
    fp8_act_quantize(scale="mxfp8") -> the grouped MX down GEMM -> fp8_moe_combine.  Six launches up to MOE_ROUTE_SINGLE_MAX assignments
    (eight beyond); nothing is read on the host; capturable into a HIP graph that replays on new ids.  Keep the weight scales in a layout the
    kernels read in place (row and expert strides multiples of 4), or every call copies them."""
    return _moe_forward("mxfp8", x, topk_ids, topk_weights, w1_q, w1_scales, w2_q, w2_scales, act, gated, bias1, bias2, out_dtype, kernel)


def fp8_moe_forward_mxfp4(x: torch.Tensor, topk_ids: torch.Tensor, topk_weights: torch.Tensor | None, w1_q: torch.Tensor, w1_scales: torch.Tensor,
                          w2_q: torch.Tensor, w2_scales: torch.Tensor, act: str = "silu", gated: bool = True, bias1: torch.Tensor | None = None,
                          bias2: torch.Tensor | None = None, out_dtype: torch.dtype | None = None, kernel: int = _l.KERNEL_AUTO) -> torch.Tensor:
    """fp8_moe_forward_mxfp8 with e2m1 elements in both GEMMs (w1_q (G, ., K/2), w2_q (G, N, H/2): fp8_quantize_mxfp4's pairs)."""
    return _moe_forward("mxfp4", x, topk_ids, topk_weights, w1_q, w1_scales, w2_q, w2_scales, act, gated, bias1, bias2, out_dtype, kernel)


def fp8_moe_forward_mxw4a8(x: torch.Tensor, topk_ids: torch.Tensor, topk_weights: torch.Tensor | None, w1_q: torch.Tensor, w1_scales: torch.Tensor,
                           w2_q: torch.Tensor, w2_scales: torch.Tensor, act: str = "silu", gated: bool = True, bias1: torch.Tensor | None = None,
                           bias2: torch.Tensor | None = None, out_dtype: torch.dtype | None = None, kernel: int = _l.KERNEL_AUTO) -> torch.Tensor:
    """fp8_moe_forward_mxfp8 against e2m1 weights in both GEMMs (w1_q (G, ., K/2), w2_q (G, N, H/2): fp8_quantize_mxfp4's pairs): the MXFP8
    layer's launches - fp8_moe_scatter_quantize(scale="mxfp8") and fp8_act_quantize(scale="mxfp8") feed the grouped MXW4A8 GEMMs."""
    return _moe_forward("mxw4a8", x, topk_ids, topk_weights, w1_q, w1_scales, w2_q, w2_scales, act, gated, bias1, bias2, out_dtype, kernel)


# ---- the gate: router logits -> topk_ids / topk_weights in one launch (include/fp8mi.h), and the layer that starts from the logits ----

_GATE_SCORING = {"softmax": _l.GATE_SOFTMAX, "sigmoid": _l.GATE_SIGMOID}
_GATE_GROUP_SCORE = {"max": _l.GATE_GROUP_MAX, "top2": _l.GATE_GROUP_TOP2}
_MOE_LAYER_RECIPE = {"rowwise": "row", "blockwise": "block128", "mxfp8": "mxfp8", "mxfp4": "mxfp4", "mxw4a8": "mxw4a8"}


def fp8_moe_gate(router_logits: torch.Tensor, k: int, scoring: str = "softmax", renormalize: bool = False, scale: float = 1.0,
                 bias: torch.Tensor | None = None, n_group: int = 1, topk_group: int = 1, group_score: str = "max"):
    """The MoE gate in one launch: (T, G) router logits -> (topk_ids int32 (T, k), topk_weights float32 (T, k)), what fp8_moe_route,
    fp8_moe_combine and fp8_moe_forward_* read.  Replaces the chain softmax / sigmoid, + bias, group mask, topk, gather, sum, div, mul, cast.

    scoring "softmax" (over all G experts, then the top-k) or "sigmoid";  bias (G,): added to the scores for the SELECTION only - the weights
    are the scores;  n_group > 1: group-limited routing, the topk_group groups with the best group score ("max": a group's largest key,
    "top2": the sum of its two largest - DeepSeek-V3) stay;  renormalize: the k weights divided by their sum (+ 1e-20);  scale multiplies them.
    Ties go to the smaller expert index, NaN ranks above +inf (torch.topk's convention); the ids of a token are always k distinct experts.
    Without bias and groups the selection runs on the logits themselves and is exact.  Logits float32 / float16 / bfloat16 with any row
    stride are read in place (a non-unit column stride is copied); other dtypes go through float32.  G <= 1024, k <= MOE_GATE_MAX_K,
    n_group <= 64."""
    assert scoring in _GATE_SCORING, f"unknown scoring {scoring!r}; expected 'softmax' or 'sigmoid'"
    assert group_score in _GATE_GROUP_SCORE, f"unknown group_score {group_score!r}; expected 'max' or 'top2'"
    assert router_logits.dim() == 2, "router_logits is (T, G)"
    assert 1 <= k <= _l.MOE_GATE_MAX_K, f"k={k}: 1 to {_l.MOE_GATE_MAX_K} experts per token"
    assert bias is None or tuple(bias.shape) == (router_logits.shape[1],), \
        f"bias has shape {tuple(bias.shape)}; one value for each of the {router_logits.shape[1]} experts is needed"
    x = _to_device(router_logits)
    if x.dtype not in _DTYPE_CODE:
        x = _TO(x, torch.float32)
    x2, T, G, ld = _rows_view(x)
    dev = x2.device
    if bias is not None:
        if not (bias.dtype is torch.float32 and bias.device == dev and bias.is_contiguous()):
            bias = _TO(bias, device=dev, dtype=torch.float32).contiguous()
    ids = torch.empty((T, k), dtype=torch.int32, device=dev)
    weights = torch.empty((T, k), dtype=torch.float32, device=dev)
    with _on_device(dev):
        rc = _l.load().fp8mi_moe_gate(x2.data_ptr(), _DTYPE_CODE[x2.dtype], T, G, ld, bias.data_ptr() if bias is not None else None, k,
                                      _GATE_SCORING[scoring], int(bool(renormalize)), float(scale), n_group, topk_group,
                                      _GATE_GROUP_SCORE[group_score], ids.data_ptr(), weights.data_ptr(), _stream(dev))
    _l.check(rc, "fp8mi_moe_gate")
    return ids, weights


def fp8_moe_layer(x: torch.Tensor, router_logits: torch.Tensor, k: int, w1: torch.Tensor, w1_scales: torch.Tensor, w2: torch.Tensor,
                  w2_scales: torch.Tensor, recipe: str = "rowwise", *, scoring: str = "softmax", renormalize: bool = False, scale: float = 1.0,
                  bias: torch.Tensor | None = None, n_group: int = 1, topk_group: int = 1, group_score: str = "max", act: str = "silu",
                  gated: bool = True, bias1: torch.Tensor | None = None, bias2: torch.Tensor | None = None, out_dtype: torch.dtype | None = None,
                  kernel: int = _l.KERNEL_AUTO) -> torch.Tensor:
    """A whole MoE layer from the router's logits: fp8_moe_gate, then fp8_moe_forward_<recipe> on its ids and weights - seven launches up to
    MOE_ROUTE_SINGLE_MAX assignments (nine beyond), nothing read on the host, capturable into a HIP graph that replays on new logits.

    x: (T, K);  router_logits: (T, G) with G = w1.shape[0];  recipe "rowwise", "blockwise", "mxfp8", "mxfp4" or "mxw4a8": the weights and scales of
    that fp8_moe_forward_*;  scoring .. group_score: fp8_moe_gate's;  act .. kernel: fp8_moe_forward_*'s.  The same bits as
    fp8_moe_forward_<recipe>(x, *fp8_moe_gate(router_logits, k, ...), ...)."""
    assert recipe in _MOE_LAYER_RECIPE, f"unknown recipe {recipe!r}; expected 'rowwise', 'blockwise', 'mxfp8' or 'mxfp4'"
    assert router_logits.dim() == 2 and x.dim() == 2 and router_logits.shape[0] == x.shape[0], "router_logits is (T, G) for x (T, K)"
    assert w1.dim() == 3 and router_logits.shape[1] == w1.shape[0], f"router_logits names {router_logits.shape[1]} experts; w1 holds {w1.shape[0]}"
    ids, weights = fp8_moe_gate(router_logits, k, scoring, renormalize, scale, bias, n_group, topk_group, group_score)
    return _moe_forward(_MOE_LAYER_RECIPE[recipe], x, ids, weights, w1, w1_scales, w2, w2_scales, act, gated, bias1, bias2, out_dtype, kernel)


# ---- the FP8 paged KV cache and single-query decode attention ----------------------------------------------------------------

# fp8mi_paged_attention_decode's and fp8mi_paged_attention_varlen's split workspaces, held like fp8mi_moe_route's: per (device, stream), the last element serves new calls
_attn_workspaces: dict = {}


def _attn_workspace(dev, stream, need: int):
    """-> a workspace of at least `need` bytes, or None while the stream is being captured and none that large exists yet (the call then
    does not split; call it once at this size before capturing)"""
    key = (dev.index, stream)
    held = _attn_workspaces.get(key)
    if held is None or held[-1].numel() < need:
        if torch.cuda.is_current_stream_capturing():
            return None
        with _workspaces_lock:
            held = _attn_workspaces.setdefault(key, [])
            if not held or held[-1].numel() < need:
                held.append(torch.empty(need, dtype=torch.uint8, device=dev))
    return held[-1]


def _kv_cache_geometry(k_cache: torch.Tensor, v_cache: torch.Tensor):
    """-> (num_blocks, Hkv, block_size, D) of a cache pair in the documented shapes"""
    assert k_cache.dtype == torch.uint8 and v_cache.dtype == torch.uint8, "the caches hold e4m3fn bytes as uint8"
    assert k_cache.dim() == 4 and v_cache.dim() == 4 and k_cache.is_contiguous() and v_cache.is_contiguous(), \
        "k_cache is a contiguous (num_blocks, Hkv, block_size, D), v_cache a contiguous (num_blocks, Hkv, D, block_size)"
    nb, Hkv, bs, D = k_cache.shape
    assert tuple(v_cache.shape) == (nb, Hkv, D, bs), f"v_cache has shape {tuple(v_cache.shape)}; k_cache {tuple(k_cache.shape)} needs {(nb, Hkv, D, bs)}"
    assert bs in _l.KV_BLOCK_SIZES and D in _l.KV_HEAD_DIMS, f"block_size {bs} / head dimension {D}: {_l.KV_BLOCK_SIZES} / {_l.KV_HEAD_DIMS} are supported"
    assert k_cache.device == v_cache.device and k_cache.device.type == DEVICE_TYPE, "both caches live on one HIP device"
    return nb, Hkv, bs, D


def _kv_scales(k_scale, v_scale, Hkv: int, dev):
    """-> (k_scale, v_scale as float32 tensors on `dev`, the scale mode): one element each, or Hkv each"""
    ks = _TO(torch.as_tensor(k_scale), device=dev, dtype=torch.float32).reshape(-1).contiguous()
    vs = _TO(torch.as_tensor(v_scale), device=dev, dtype=torch.float32).reshape(-1).contiguous()
    assert ks.numel() == vs.numel() and ks.numel() in (1, Hkv), f"k_scale and v_scale hold one value each or one per KV head ({Hkv}) each"
    return ks, vs, (_l.KV_SCALE_HEAD if ks.numel() == Hkv and Hkv > 1 else _l.KV_SCALE_TENSOR)


def _heads_view(x: torch.Tensor, H: int, D: int, what: str) -> torch.Tensor:
    """x (rows, H, D) on the device in a dtype the kernels read, used in place when a row's heads are contiguous (a slice of a fused qkv)"""
    assert x.dim() == 3 and tuple(x.shape[1:]) == (H, D), f"{what} has shape {tuple(x.shape)}; (rows, {H}, {D}) is needed"
    x = _float_source(x)
    if not (x.stride(2) == 1 and x.stride(1) == D and (x.shape[0] <= 1 or x.stride(0) >= H * D)):
        x = x.contiguous()
    return x


def fp8_kv_cache_alloc(num_blocks: int, block_size: int, Hkv: int, D: int, device=DEVICE_TYPE):
    """-> (k_cache uint8 (num_blocks, Hkv, block_size, D), v_cache uint8 (num_blocks, Hkv, D, block_size)), zeroed: e4m3fn bytes.  In the V
    cache a channel's positions are contiguous, which is how fp8_paged_attention's P.V product reads them."""
    assert block_size in _l.KV_BLOCK_SIZES and D in _l.KV_HEAD_DIMS, f"block_size {block_size} / D {D}: {_l.KV_BLOCK_SIZES} / {_l.KV_HEAD_DIMS} are supported"
    assert num_blocks >= 0 and Hkv >= 1
    return (torch.zeros((num_blocks, Hkv, block_size, D), dtype=torch.uint8, device=device),
            torch.zeros((num_blocks, Hkv, D, block_size), dtype=torch.uint8, device=device))


def fp8_kv_cache_append(k: torch.Tensor, v: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, slot_mapping: torch.Tensor, k_scale, v_scale,
                        encode_mode: int | None = None) -> None:
    """Quantise T new tokens' k, v (T, Hkv, D) to e4m3 with the static dequantisation scales k_scale, v_scale (one value each, or (Hkv,)
    each) and write them to slot slot_mapping[t] = block * block_size + offset of both caches, in one launch: the bytes of
    fp8_encode(x * (1 / scale)).  A negative slot is padding.  k and v may be slices of one fused qkv tensor (read in place); nothing is
    read on the host."""
    nb, Hkv, bs, D = _kv_cache_geometry(k_cache, v_cache)
    dev = k_cache.device
    k, v = _heads_view(_TO(k, device=dev), Hkv, D, "k"), _heads_view(_TO(v, device=dev), Hkv, D, "v")
    assert k.shape[0] == v.shape[0], "k and v hold the same tokens"
    if k.dtype != v.dtype:
        k, v = _TO(k, torch.float32), _TO(v, torch.float32)
    T = k.shape[0]
    slots = _TO(slot_mapping, device=dev).reshape(-1)
    if slots.dtype not in (torch.int32, torch.int64):
        slots = _TO(slots, torch.int64)
    slots = slots.contiguous()
    assert slots.numel() == T, f"slot_mapping names {slots.numel()} slots for {T} tokens"
    ks, vs, mode = _kv_scales(k_scale, v_scale, Hkv, dev)
    _call("fp8mi_kv_cache_append", dev, k.data_ptr(), v.data_ptr(), _DTYPE_CODE[k.dtype], T, Hkv, D, k.stride(0) if T > 1 else Hkv * D,
          v.stride(0) if T > 1 else Hkv * D, k_cache.data_ptr(), v_cache.data_ptr(), nb, bs, slots.data_ptr(), slots.element_size(), ks.data_ptr(),
          vs.data_ptr(), mode, ENCODE_MODE if encode_mode is None else encode_mode)


def fp8_paged_attention(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, block_table: torch.Tensor, seq_lens: torch.Tensor, k_scale,
                        v_scale, softmax_scale: float | None = None, max_seq_len: int | None = None, num_splits: int = 0,
                        out_dtype: torch.dtype | None = None, workspace: torch.Tensor | None = None, cu_seqlens_q: torch.Tensor | None = None,
                        max_q_len: int | None = None) -> torch.Tensor:
    """Single-query attention over the FP8 paged KV cache: q (B, Hq, D), one token per sequence, against positions [0, seq_lens[b]) of the
    blocks block_table[b] names -> (B, Hq, D) in out_dtype (default q's).  Hq is a multiple of Hkv, at most 16 query heads to a KV head.
    softmax_scale defaults to D ** -0.5.  max_seq_len is a host upper bound of seq_lens that sizes the grid (default: all the table can
    name) - seq_lens itself is never read on the host, so the call is capturable and replays on new lengths, tables and cache contents.
    num_splits 0: chosen by the library; 1: one launch; n: n splits of the positions, two launches.  Nothing outside [0, seq_len) - the tail
    of the last block, blocks beyond the need, whatever their bytes - influences the output; seq_len == 0 gives a zero row.

    With cu_seqlens_q (int32 (B + 1,), B = block_table.shape[0]) the multi-token form (fp8mi_paged_attention_varlen): q is (T, Hq, D),
    sequence b owns the rows [cu[b], cu[b + 1]), already appended to the cache and counted in seq_lens[b]; token j of q_len_b attends the
    positions [0, seq_lens[b] - q_len_b + j + 1) - causal, aligned at the end of the context.  max_q_len is a host upper bound of q_len_b
    (default T).  Rows no sequence owns, and a sequence's rows at or beyond max_q_len, are not written: they are whatever torch.empty held."""
    nb, Hkv, bs, D = _kv_cache_geometry(k_cache, v_cache)
    dev = k_cache.device
    varlen = cu_seqlens_q is not None
    assert varlen or max_q_len is None, "max_q_len belongs to cu_seqlens_q"
    assert q.dim() == 3 and q.shape[2] == D and q.shape[1] % Hkv == 0, f"q has shape {tuple(q.shape)}; (B, a multiple of {Hkv}, {D}) is needed"
    R, Hq = q.shape[0], q.shape[1]   # query rows: B, or T with cu_seqlens_q
    B = block_table.shape[0] if varlen else R
    assert Hq // Hkv <= _l.ATTN_MAX_GROUP, f"Hq / Hkv = {Hq // Hkv}; at most {_l.ATTN_MAX_GROUP} query heads share a KV head"
    assert 0 <= num_splits <= _l.ATTN_MAX_SPLITS, f"num_splits={num_splits}: 0 (chosen by the library) to {_l.ATTN_MAX_SPLITS}"
    q = _heads_view(_TO(q, device=dev), Hq, D, "q")
    out_dtype = q.dtype if out_dtype is None else out_dtype
    assert block_table.dim() == 2 and block_table.shape[0] == B and tuple(seq_lens.shape) == (B,), "block_table is (B, max_blocks), seq_lens (B,)"
    if not (block_table.dtype is torch.int32 and block_table.device == dev and block_table.stride(1) == 1):
        block_table = _TO(block_table, device=dev, dtype=torch.int32).contiguous()
    if not (seq_lens.dtype is torch.int32 and seq_lens.device == dev and seq_lens.is_contiguous()):
        seq_lens = _TO(seq_lens, device=dev, dtype=torch.int32).contiguous()
    if varlen:
        assert tuple(cu_seqlens_q.shape) == (B + 1,), f"cu_seqlens_q has shape {tuple(cu_seqlens_q.shape)}; ({B + 1},) is needed"
        if not (cu_seqlens_q.dtype is torch.int32 and cu_seqlens_q.device == dev and cu_seqlens_q.is_contiguous()):
            cu_seqlens_q = _TO(cu_seqlens_q, device=dev, dtype=torch.int32).contiguous()
        max_q_len = R if max_q_len is None else int(max_q_len)
        assert max_q_len >= 0, f"max_q_len={max_q_len}"
    max_blocks = block_table.shape[1]
    max_seq_len = max_blocks * bs if max_seq_len is None else min(int(max_seq_len), max_blocks * bs)
    ks, vs, mode = _kv_scales(k_scale, v_scale, Hkv, dev)
    out = torch.empty((R, Hq, D), dtype=out_dtype, device=dev)
    lib = _l.load()
    with _on_device(dev):
        stream = _stream(dev)
        if workspace is None and num_splits != 1:
            need = int(lib.fp8mi_paged_attention_workspace_bytes(R, Hq, D, num_splits))
            workspace = _attn_workspace(dev, stream, need) if need else None
            assert workspace is not None or num_splits == 0 or need == 0, \
                "fp8_paged_attention: a forced split needs a workspace; pass workspace=, or call it once on this stream before capturing"
        cache = (k_cache.data_ptr(), v_cache.data_ptr(), nb, bs, block_table.data_ptr(), block_table.stride(0) if B > 1 else max_blocks, max_blocks,
                 seq_lens.data_ptr(), max_seq_len, ks.data_ptr(), vs.data_ptr(), mode, float(D ** -0.5 if softmax_scale is None else softmax_scale), num_splits,
                 workspace.data_ptr() if workspace is not None else None, workspace.numel() * workspace.element_size() if workspace is not None else 0,
                 out.data_ptr(), _out_code(out_dtype), Hq * D, stream)
        ld_q = q.stride(0) if R > 1 else Hq * D
        if varlen:
            fn = "fp8mi_paged_attention_varlen"
            rc = lib.fp8mi_paged_attention_varlen(q.data_ptr(), _DTYPE_CODE[q.dtype], R, B, cu_seqlens_q.data_ptr(), max_q_len, Hq, Hkv, D, ld_q, *cache)
        else:
            fn = "fp8mi_paged_attention_decode"
            rc = lib.fp8mi_paged_attention_decode(q.data_ptr(), _DTYPE_CODE[q.dtype], B, Hq, Hkv, D, ld_q, *cache)
    _l.check(rc, fn)
    return out


def scaled_grouped_mm_colmajor(input: torch.Tensor, mat2: torch.Tensor, scale_a: torch.Tensor, scale_b: torch.Tensor, offs: torch.Tensor, out_dtype=None):
    """The 2D x 3D call torch._scaled_grouped_mm makes, without intermediate tensors: `input` (M_total, K) row-major, `mat2` (G, K, N) with every
    expert column-major - its storage then already is the (G, N, K) operand the kernels read.  Returns None for any other layout."""
    if input.dim() != 2 or mat2.dim() != 3 or mat2.shape[1] != input.shape[1] or mat2.device != input.device:
        return None
    M, K = input.shape
    G, _k, N = mat2.shape
    if G < 1 or K == 0 or not (input.stride(1) == 1 and input.stride(0) >= K):
        return None
    if not (mat2.stride(1) == 1 and mat2.stride(2) >= K and (G == 1 or mat2.stride(0) >= (N - 1) * mat2.stride(2) + K)):
        return None
    return fp8_scaled_mm_grouped(input, mat2.transpose(1, 2), scale_a, scale_b, offs, out_dtype=out_dtype)


def fp8_mlp_mxfp8(x: torch.Tensor, w1_q: torch.Tensor, w1_scales: torch.Tensor, w2_q: torch.Tensor, w2_scales: torch.Tensor, act: str = "silu",
                  gated: bool = True, bias1: torch.Tensor | None = None, bias2: torch.Tensor | None = None,
                  out_dtype: torch.dtype | None = None) -> torch.Tensor:
    """fp8_mlp_blockwise on the MXFP8 recipe: one E8M0 scale per 32 features of every row of both operands of both GEMMs.  x is quantised
    by the streaming kernel (act="none", scale="mxfp8": the bytes and scales of fp8_quantize_mxfp8(x)), the first GEMM writes h in x's
    dtype, the hidden activations go through the same kernel with `act` (and the gate product), then the second GEMM.

    x: (..., K), K % 32 == 0;  w1_q: (H, K) - (2H, K) when gated, rows [gate | up] - e4m3fn bytes with (rows, K/32) E8M0 scales
    (fp8_quantize_mxfp8 of the weight);  w2_q: (N, H), H % 32 == 0."""
    return _dense_mlp("mxfp8", x, w1_q, w1_scales, w2_q, w2_scales, act, gated, bias1, bias2, out_dtype)


def fp8_mlp_mxfp4(x: torch.Tensor, w1_q: torch.Tensor, w1_scales: torch.Tensor, w2_q: torch.Tensor, w2_scales: torch.Tensor, act: str = "silu",
                  gated: bool = True, bias1: torch.Tensor | None = None, bias2: torch.Tensor | None = None,
                  out_dtype: torch.dtype | None = None) -> torch.Tensor:
    """fp8_mlp_mxfp8 with e2m1 elements: w1_q (H, K/2) - (2H, K/2) when gated - and w2_q (N, H/2) are fp8_quantize_mxfp4's pairs."""
    return _dense_mlp("mxfp4", x, w1_q, w1_scales, w2_q, w2_scales, act, gated, bias1, bias2, out_dtype)


def fp8_mlp_mxw4a8(x: torch.Tensor, w1_q: torch.Tensor, w1_scales: torch.Tensor, w2_q: torch.Tensor, w2_scales: torch.Tensor, act: str = "silu",
                   gated: bool = True, bias1: torch.Tensor | None = None, bias2: torch.Tensor | None = None,
                   out_dtype: torch.dtype | None = None) -> torch.Tensor:
    """fp8_mlp_mxfp8 against e2m1 weights: x and the hidden activations are quantised to MXFP8 by the same two launches, w1_q (H, K/2) -
    (2H, K/2) when gated - and w2_q (N, H/2) are fp8_quantize_mxfp4's pairs."""
    return _dense_mlp("mxw4a8", x, w1_q, w1_scales, w2_q, w2_scales, act, gated, bias1, bias2, out_dtype)


# ---- fused RMSNorm / LayerNorm (+ residual, affine parameters, adaLN modulation) + quantisation, and the linears behind it (include/fp8mi.h) ----

_NORM_CODE = {"rms": _l.NORM_RMS, "layer": _l.NORM_LAYER}


def fp8_norm_quantize(x: torch.Tensor, norm: str = "rms", weight: torch.Tensor | None = None, bias: torch.Tensor | None = None, eps: float = 1e-6,
                      residual: torch.Tensor | None = None, mod_scale: torch.Tensor | None = None, mod_shift: torch.Tensor | None = None,
                      scale: str = "row", out_format: int = _l.FMT_E4M3, encode_mode: int | None = None, return_stats: bool = False):
    """The normalised hidden state of a transformer block as an FP8 GEMM operand, in ONE launch:  h = x (+ residual, rounded to x's dtype),
    d = h (norm="rms") or h - mean(h) ("layer"), rstd = 1 / sqrt(mean(d^2) + eps),  y = d * rstd [* weight] [+ bias]
    [* (1 + mod_scale) + mod_shift], every step one fp32 operation (include/fp8mi.h: fp8mi_norm_quantize), and y quantised as
    fp8_act_quantize quantises - without y ever reaching memory.

    x: (..., C) float32 / float16 / bfloat16; a 2-D column-slice view is read in place through its row stride.  weight, bias: (C,).
    residual: x's shape and dtype.  mod_scale, mod_shift: (B, C) or (B, 1, C) for x of (B, ..., C) - adaLN's one row per image, used by
    all of its tokens.  The parameters share one dtype: x's or float32.  Returns (q, scales) shaped and typed as fp8_act_quantize's for
    `scale` ("row" | "block128" | "mxfp8" | "mxfp4"), `out_format` and `encode_mode`; then h (x's shape and dtype) when a residual is given; then, with
    return_stats, rstd and - for "layer" - mean, float32 of shape (..., 1): the values every element was computed with."""
    assert norm in _NORM_CODE, f"unknown norm {norm!r}; expected one of {sorted(_NORM_CODE)}"
    recipe = _scale_recipe(scale, out_format, encode_mode)
    assert (mod_scale is None) == (mod_shift is None), "mod_scale and mod_shift come together"
    assert x.dim() >= 1, "takes a (..., C) tensor"
    x = _float_source(x)
    lead = tuple(x.shape[:-1])
    x2, rows, cols, ld_in = _rows_view(x)
    dev = x2.device
    params = [t for t in (weight, bias, mod_scale, mod_shift) if t is not None]
    pdt = params[0].dtype if params else x2.dtype
    assert all(t.dtype == pdt for t in params), f"the parameters share one dtype, not {[t.dtype for t in params]}"
    assert pdt in (x2.dtype, torch.float32), f"the parameters are {x2.dtype} like x, or float32, not {pdt}"
    for name, t in (("weight", weight), ("bias", bias)):
        assert t is None or tuple(t.shape) == (cols,), f"{name} has shape {tuple(t.shape)}; expected ({cols},)"
    weight, bias = (None if t is None else _to_device(t).contiguous() for t in (weight, bias))
    ld_mod, rows_per_mod = max(cols, 1), 1
    if mod_scale is not None:
        assert x.dim() >= 2, "modulation takes x of (B, ..., C)"
        B = x.shape[0]
        ok = ((B, cols), (B, 1, cols))
        assert tuple(mod_scale.shape) in ok and tuple(mod_shift.shape) in ok, \
            f"mod_scale / mod_shift have shapes {tuple(mod_scale.shape)} / {tuple(mod_shift.shape)}; expected {ok[0]} or {ok[1]}"
        mod_scale, mod_shift = (_to_device(t).reshape(B, cols).contiguous() for t in (mod_scale, mod_shift))
        rows_per_mod = max(rows // B, 1) if B else 1
    ld_res, h = max(cols, 1), None
    if residual is not None:
        assert residual.shape == x.shape and residual.dtype == x.dtype, \
            f"residual is {tuple(residual.shape)} {residual.dtype}; expected x's {tuple(x.shape)} {x.dtype}"
        res2, _, _, ld_res = _rows_view(_to_device(residual))
        h = torch.empty((rows, cols), dtype=x2.dtype, device=dev)
    layer = norm == "layer"
    rstd = torch.empty((rows,), dtype=torch.float32, device=dev) if return_stats else None
    mean = torch.empty((rows,), dtype=torch.float32, device=dev) if return_stats and layer else None
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    # the input, the normalisation and its parameters, the residual stream, then q and its scales (no amax output here), then the statistics
    args, q, sc = _scale_outputs(recipe, rows, cols, dev, (None,))
    _call("fp8mi_norm_quantize" + recipe[3], dev, x2.data_ptr(), _DTYPE_CODE[x2.dtype], rows, cols, ld_in, _NORM_CODE[norm], float(eps), ptr(weight),
          ptr(bias), ptr(mod_scale), ptr(mod_shift), ld_mod, rows_per_mod, _DTYPE_CODE[pdt], res2.data_ptr() if residual is not None else None, ld_res,
          ptr(h), max(cols, 1), *args, ptr(mean), ptr(rstd))
    out = list(_scale_results(recipe, q, sc, lead, cols))
    if h is not None:
        out.append(h.reshape(*lead, cols))
    if return_stats:
        out.append(rstd.reshape(*lead, 1))
        if layer:
            out.append(mean.reshape(*lead, 1))
    return tuple(out)


def fp8_norm_linear_rowwise(x: torch.Tensor, w: torch.Tensor, w_scale: torch.Tensor, norm: str = "rms", weight: torch.Tensor | None = None,
                            norm_bias: torch.Tensor | None = None, eps: float = 1e-6, residual: torch.Tensor | None = None,
                            mod_scale: torch.Tensor | None = None, mod_shift: torch.Tensor | None = None, bias: torch.Tensor | None = None,
                            out_dtype: torch.dtype | None = None):
    """linear(norm(x)) with the normalised activations never leaving FP8: the fused launch of fp8_norm_quantize (one scale per token), then
    the GEMM call of fp8_linear_rowwise.  w: (N, K) e4m3fn bytes (or e5m2);  w_scale: [1] or one per output channel;  `weight`,
    `norm_bias`, `mod_*`, `residual`: the normalisation's, as in fp8_norm_quantize;  `bias`: the linear's.  Returns (..., N) in `out_dtype`
    (default x.dtype, float32 for other inputs) - and h = x + residual as a second value when a residual is given."""
    return _dense_norm_linear("row", x, w, w_scale, norm, weight, norm_bias, eps, residual, mod_scale, mod_shift, bias, out_dtype)


def fp8_norm_linear_blockwise(x: torch.Tensor, w_q: torch.Tensor, w_scales: torch.Tensor, norm: str = "rms", weight: torch.Tensor | None = None,
                              norm_bias: torch.Tensor | None = None, eps: float = 1e-6, residual: torch.Tensor | None = None,
                              mod_scale: torch.Tensor | None = None, mod_shift: torch.Tensor | None = None, bias: torch.Tensor | None = None,
                              out_dtype: torch.dtype | None = None):
    """fp8_norm_linear_rowwise on the blockwise (DeepSeek) recipe: 1x128 activation scales from the fused launch against 128x128 weight
    scales - the GEMM call of fp8_mlp_blockwise's first layer.  w_q: (N, K) e4m3fn bytes;  w_scales: (ceil(N/128), ceil(K/128))."""
    return _dense_norm_linear("block128", x, w_q, w_scales, norm, weight, norm_bias, eps, residual, mod_scale, mod_shift, bias, out_dtype)


def fp8_norm_linear_mxfp8(x: torch.Tensor, w_q: torch.Tensor, w_scales: torch.Tensor, norm: str = "rms", weight: torch.Tensor | None = None,
                          norm_bias: torch.Tensor | None = None, eps: float = 1e-6, residual: torch.Tensor | None = None,
                          mod_scale: torch.Tensor | None = None, mod_shift: torch.Tensor | None = None, bias: torch.Tensor | None = None,
                          out_dtype: torch.dtype | None = None):
    """fp8_norm_linear_blockwise on the MXFP8 recipe: E8M0 scales per 32 features from the fused launch (fp8_norm_quantize, scale="mxfp8"),
    then the GEMM call of fp8_linear_mxfp8.  w_q: (N, K) e4m3fn bytes;  w_scales: (N, K/32) E8M0;  K % 32 == 0.  Returns y - and
    h = x + residual as a second value when a residual is given."""
    return _dense_norm_linear("mxfp8", x, w_q, w_scales, norm, weight, norm_bias, eps, residual, mod_scale, mod_shift, bias, out_dtype)


def fp8_norm_linear_mxfp4(x: torch.Tensor, w_q: torch.Tensor, w_scales: torch.Tensor, norm: str = "rms", weight: torch.Tensor | None = None,
                          norm_bias: torch.Tensor | None = None, eps: float = 1e-6, residual: torch.Tensor | None = None,
                          mod_scale: torch.Tensor | None = None, mod_shift: torch.Tensor | None = None, bias: torch.Tensor | None = None,
                          out_dtype: torch.dtype | None = None):
    """fp8_norm_linear_mxfp8 with e2m1 elements: w_q (N, K/2) is fp8_quantize_mxfp4's pairs."""
    return _dense_norm_linear("mxfp4", x, w_q, w_scales, norm, weight, norm_bias, eps, residual, mod_scale, mod_shift, bias, out_dtype)


def fp8_norm_linear_mxw4a8(x: torch.Tensor, w_q: torch.Tensor, w_scales: torch.Tensor, norm: str = "rms", weight: torch.Tensor | None = None,
                           norm_bias: torch.Tensor | None = None, eps: float = 1e-6, residual: torch.Tensor | None = None,
                           mod_scale: torch.Tensor | None = None, mod_shift: torch.Tensor | None = None, bias: torch.Tensor | None = None,
                           out_dtype: torch.dtype | None = None):
    """fp8_norm_linear_mxfp8 against e2m1 weights: the fused launch quantises to MXFP8 (scale="mxfp8"), w_q (N, K/2) is
    fp8_quantize_mxfp4's pairs."""
    return _dense_norm_linear("mxw4a8", x, w_q, w_scales, norm, weight, norm_bias, eps, residual, mod_scale, mod_shift, bias, out_dtype)


def pad_weight_rows(weight: torch.Tensor, pad_bytes: int = 256) -> torch.Tensor:
    """The same (N, K) fp8 / uint8 weight in a buffer whose ROW STRIDE is K + pad_bytes (a one-time copy at load time).  No counterpart
    in the reference (its kernels take no strides); the C ABI and every Python entry point here take the stride as it is (`ldb`):
    pass the returned view, or its `.t()` to the patched torch._scaled_mm.  Results are bit-identical to the unpadded call.

    Why: the small-batch tile kernels stream W as 8-row x 128-byte pieces, and with some power-of-two-ish row strides those pieces
    crowd onto few memory channels.  Measured on MI355X for M <= 128 (tools/sweep_pad.py, profiles/r03_row_stride.txt), +256 bytes:
    K = 16384, N = 4096: 18.5 -> 14.3 us at M = 16 (19.6 -> 16.0 at M = 64); K = N = 8192: 14.2 -> 12.4 (18.1 -> 16.8);
    K = N = 16384: 55.6 -> 45.9; K = 20480, N = 4096: 21.0 -> 17.0 at M = 64.  It is NOT a rule of K alone: K = 8192 against
    N = 4096 or 14336, K = 4096, 14336, 24576, 28672 and every M >= 512 do not change, and K = 32768 gets 23 % SLOWER with 256
    (unchanged with 512).  Measure the deployment's shapes with tools/sweep_pad.py before padding a model's weights."""
    assert weight.dim() == 2 and weight.element_size() == 1, "an (N, K) matrix of fp8 bytes"
    assert pad_bytes >= 0 and pad_bytes % 16 == 0, "the tile kernels need 16-byte aligned rows"
    if pad_bytes == 0:
        return weight
    N, K = weight.shape
    buf = torch.empty((N, K + pad_bytes), dtype=torch.uint8, device=weight.device)
    view = buf[:, :K]
    view.copy_(weight.view(torch.uint8) if weight.dtype != torch.uint8 else weight)
    return view if weight.dtype == torch.uint8 else view.view(weight.dtype)


def fp8_amax(input: torch.Tensor) -> torch.Tensor:
    """max|input| as a float32[1] device tensor (no host sync)."""
    inp, code, _ = _encode_source(input, result=False)
    out = torch.empty(1, dtype=torch.float32, device=inp.device)
    _call("fp8mi_amax", inp.device, inp.data_ptr(), code, out.data_ptr(), inp.numel())
    return out


def fp8_scaled_mm_auto(A, B, scale_a, scale_b, **kw):
    """Shape-based strategy choice (fp8_mps_native.py:193-210).  The reference
    switches at M <= 16 between its fused kernel and a dequant + fp16 matmul;
    here the choice (GEMV / MFMA GEMM tile shape / generic) is made inside
    fp8mi_scaled_mm from M, N, K and alignment."""
    return fp8_scaled_mm(A, B, scale_a, scale_b, **kw)


# The reference's "fast" path (fp8_mps_native.py:213-267) dequantises both
# operands to fp16 and calls the native matmul.  On gfx950 that would be slower
# and less accurate than the fp8 MFMA kernel, so the name maps to the same op.
fp8_scaled_mm_fast = fp8_scaled_mm
