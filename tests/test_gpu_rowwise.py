"""GPU: per-row dynamic quantisation (fp8mi_quantize_rowwise), its dequantisation, fp8_linear_rowwise, the _scaled_mm route on the
quantiser's outputs, graph capture and the C ABI, against tests/rowwise_ref.py.

Every comparison against the reference is byte for byte, and bit for bit for the float32 scales: there are no tolerances in this file."""
import os
import subprocess

import numpy as np
import pytest
import torch

import fp8_mi355x_lib as L
import rowwise_ref as R
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

E4, E5 = L.FMT_E4M3, L.FMT_E5M2
CODE = {torch.float32: L.F32, torch.float16: L.F16, torch.bfloat16: L.BF16}
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
ENCS = [(E4, L.ENC_REFERENCE), (E4, L.ENC_RNE), (E5, L.ENC_RNE)]
ENC_IDS = ["e4m3-reference", "e4m3-rne", "e5m2"]
COLS = [1, 7, 16, 100, 1024, 3072, 4100, 14336, 16384, 16400, 40000]
ROWS = [1, 3, 64, 257]


def make(rng, rows, cols, dt):
    """N(0,1) rows with magnitudes spread over 2^-8 .. 2^7 (inside float16's range), in dtype dt."""
    x = rng.standard_normal((rows, cols)) * np.exp2(rng.integers(-8, 8, size=(rows, 1)))
    return torch.from_numpy(x.astype(np.float32)).to(dt)


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def check_q(q, inv, amax, x, fmt, mode, what=""):
    """q / inv / amax (device tensors; amax may be None) against the reference of the 2-D host tensor x."""
    wq, wamax, winv = R.quantize_rowwise_ref(x, fmt, mode)
    g = q.view(torch.uint8).cpu().numpy().reshape(wq.shape)
    bad = np.argwhere(g != wq)
    assert bad.shape[0] == 0, (what, bad.shape[0], [(int(r), int(c), hex(int(g[r, c])), hex(int(wq[r, c]))) for r, c in bad[:6]])
    gi = inv.cpu().numpy().reshape(-1)
    assert np.array_equal(bits(gi), bits(winv)), (what, "inv", gi[:4], winv[:4])
    if amax is not None:
        assert np.array_equal(bits(amax.cpu().numpy().reshape(-1)), bits(wamax)), (what, "amax")


def raw_quantize(x_ptr, dt, rows, cols, ld_in, out_ptr, ld_out, inv_ptr, amax_ptr, fmt, mode):
    rc = L.load().fp8mi_quantize_rowwise(x_ptr, CODE[dt], rows, cols, ld_in, out_ptr, ld_out, inv_ptr, amax_ptr, fmt, mode,
                                         torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.load().fp8mi_last_error()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# quantiser: the full grid
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,mode", ENCS, ids=ENC_IDS)
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f16", "bf16"])
def test_quantize_rowwise_grid(native, cuda, dt, fmt, mode):
    """Every register form (one wave per row, four / eight waves per row), the looping form (16400 and 40000 columns), the scalar form
    (rows that are not 16-byte multiples: 1, 7, 100, 4100 ... columns with more than one row) and the per-row tails."""
    rng = np.random.default_rng(100 * CODE[dt] + 10 * fmt + mode)
    for cols in COLS:
        for rows in ROWS:
            x = make(rng, rows, cols, dt)
            q, inv, amax = native.fp8_quantize_rowwise(x.to(cuda), out_format=fmt, encode_mode=mode, return_amax=True)
            assert q.shape == x.shape and inv.shape == (rows, 1) and amax.shape == (rows, 1) and inv.dtype == torch.float32
            assert q.dtype == (torch.float8_e5m2 if fmt == E5 else torch.uint8)
            check_q(q, inv, amax, x, fmt, mode, what=f"{dt} {rows}x{cols}")


def test_quantize_rowwise_shapes_and_defaults(native, cuda):
    rng = np.random.default_rng(7)
    x = make(rng, 12, 512, torch.bfloat16).reshape(3, 4, 512)
    q, inv = native.fp8_quantize_rowwise(x.to(cuda))
    assert q.shape == (3, 4, 512) and q.dtype == torch.uint8 and inv.shape == (3, 4, 1)
    check_q(q, inv, None, x.reshape(12, 512), E4, native.ENCODE_MODE, "3-D, module default mode")
    q, inv = native.fp8_quantize_rowwise(x.to(cuda), out_format=E5)
    assert q.dtype == torch.float8_e5m2
    check_q(q, inv, None, x.reshape(12, 512), E5, L.ENC_RNE, "e5m2 default mode")
    v = make(rng, 1, 300, torch.float32).reshape(300)
    q, inv = native.fp8_quantize_rowwise(v.to(cuda))
    assert q.shape == (300,) and inv.shape == (1,)
    check_q(q, inv, None, v.reshape(1, 300), E4, native.ENCODE_MODE, "1-D")
    xi = torch.arange(-40, 40, dtype=torch.int32).reshape(4, 20)          # other dtypes are widened to float32 first
    q, inv = native.fp8_quantize_rowwise(xi.to(cuda))
    check_q(q, inv, None, xi.float(), E4, native.ENCODE_MODE, "int32")
    with pytest.raises(L.Fp8miError):
        native.fp8_quantize_rowwise(x.to(cuda), out_format=E5, encode_mode=L.ENC_REFERENCE)


# ---------------------------------------------------------------------------------------------------------------------------
# quantiser: edge inputs
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt,fmt,mode", [(torch.bfloat16, E4, L.ENC_REFERENCE), (torch.float32, E4, L.ENC_RNE), (torch.float16, E5, L.ENC_RNE)],
                         ids=["bf16-ref", "f32-rne", "f16-e5m2"])
def test_leading_dimensions_and_untouched_padding(cuda, dt, fmt, mode):
    rng = np.random.default_rng(11 + fmt + mode)
    # (cols, ld_in, ld_out): aligned strides (vector forms), odd strides (scalar form), long rows (looping form)
    for rows, cols, ld_in, ld_out in ((37, 1000, 1024, 1008), (37, 1000, 1001, 1003), (5, 3072, 4096, 3072), (5, 3072, 3072, 3080),
                                      (3, 20000, 20480, 20016), (2, 20000, 20001, 20000), (9, 16, 16, 17), (4, 12288, 12296, 12304)):
        x = make(rng, rows, ld_in, dt)
        xd = x.to(cuda)
        out = torch.full((rows, ld_out), 0xA5, dtype=torch.uint8, device=cuda)
        inv = torch.empty(rows, dtype=torch.float32, device=cuda)
        amax = torch.empty(rows, dtype=torch.float32, device=cuda)
        raw_quantize(xd.data_ptr(), dt, rows, cols, ld_in, out.data_ptr(), ld_out, inv.data_ptr(), amax.data_ptr(), fmt, mode)
        check_q(out[:, :cols].contiguous(), inv, amax, x[:, :cols], fmt, mode, what=f"{rows}x{cols} ld_in {ld_in} ld_out {ld_out}")
        assert out[:, cols:].eq(0xA5).all(), (rows, cols, ld_in, ld_out, "padding bytes written")


@pytest.mark.parametrize("dt,fmt,mode", [(torch.bfloat16, E4, L.ENC_RNE), (torch.float32, E4, L.ENC_REFERENCE), (torch.float16, E5, L.ENC_RNE)],
                         ids=["bf16-rne", "f32-ref", "f16-e5m2"])
def test_pointers_offset_by_one_and_two_elements(cuda, dt, fmt, mode):
    """Input and output pointers that are not 16- / 8-byte aligned take the scalar form; the bytes in front of and behind the output
    stay what they were."""
    rng = np.random.default_rng(21 + fmt + mode)
    esz = torch.empty(0, dtype=dt).element_size()
    for rows, cols in ((1, 5000), (6, 1024), (3, 17000), (5, 33)):
        for off_in, off_out in ((1, 0), (0, 1), (1, 1), (2, 2), (2, 0)):
            x = make(rng, rows, cols, dt)
            buf = torch.zeros(rows * cols + 8, dtype=dt, device=cuda)
            buf[off_in:off_in + rows * cols].copy_(x.reshape(-1).to(cuda))
            out = torch.full((rows * cols + 16,), 0x5A, dtype=torch.uint8, device=cuda)
            inv = torch.empty(rows, dtype=torch.float32, device=cuda)
            raw_quantize(buf.data_ptr() + off_in * esz, dt, rows, cols, cols, out.data_ptr() + off_out, cols, inv.data_ptr(), None, fmt, mode)
            check_q(out[off_out:off_out + rows * cols].contiguous(), inv, None, x, fmt, mode, what=f"{rows}x{cols} offsets {off_in} {off_out}")
            assert out[:off_out].eq(0x5A).all() and out[off_out + rows * cols:].eq(0x5A).all()


def test_column_slice_view_through_the_python_op(native, cuda):
    rng = np.random.default_rng(31)
    wide = make(rng, 40, 4096, torch.bfloat16)
    wd = wide.to(cuda)
    for c0, cols in ((512, 3072), (8, 1024), (3, 100), (1, 4095), (0, 4096)):
        for fmt, mode in ENCS:
            q, inv, amax = native.fp8_quantize_rowwise(wd[:, c0:c0 + cols], out_format=fmt, encode_mode=mode, return_amax=True)
            assert q.is_contiguous() and q.shape == (40, cols)
            check_q(q, inv, amax, wide[:, c0:c0 + cols], fmt, mode, what=f"slice {c0}+{cols}")
    # a transposed view is copied
    t = wd[:, :64].t()
    q, inv = native.fp8_quantize_rowwise(t, encode_mode=L.ENC_RNE)
    check_q(q, inv, None, wide[:, :64].t().contiguous(), E4, L.ENC_RNE, "transposed view")


@pytest.mark.parametrize("fmt,mode", ENCS, ids=ENC_IDS)
def test_zero_rows_nan_rows_and_inf_rows(native, cuda, fmt, mode):
    rng = np.random.default_rng(41 + fmt + mode)
    for dt, cols in ((torch.float32, 777), (torch.bfloat16, 3072), (torch.float16, 12288), (torch.bfloat16, 20000), (torch.float32, 50)):
        x = make(rng, 12, cols, dt)
        x[1] = 0.0                                   # all-zero rows among non-zero ones: scale 1, bytes 0
        x[7] = 0.0
        x[7, cols // 2] = -0.0
        x[3, 5] = float("nan")                       # NaNs are ignored by the amax and encoded as the mode says
        x[3, cols - 1] = -float("nan")
        x[4] = float("nan")                          # a row of nothing but NaNs: amax 0, scale 1
        x[5, 0] = float("nan")                       # the row's largest magnitude right next to a NaN
        x[5, 1] = 3.0e4
        x[8, 9] = float("inf")                       # an infinite amax: scale 0, inverse scale inf, inf * 0 = NaN
        x[9, cols - 2] = float("-inf")
        x[10, 3], x[10, 4] = float("inf"), float("nan")
        q, inv, amax = native.fp8_quantize_rowwise(x.to(cuda), out_format=fmt, encode_mode=mode, return_amax=True)
        check_q(q, inv, amax, x, fmt, mode, what=f"specials {dt} {cols}")
        g = q.view(torch.uint8).cpu()
        assert g[1].eq(0).all() and inv[1].item() == 1.0 and amax[1].item() == 0.0
        assert inv[4].item() == 1.0 and amax[4].item() == 0.0 and (g[4] & 0x7F).eq(0x7F).all()
        assert amax[5].item() == 3.0e4 if dt != torch.bfloat16 else amax[5].item() == float(torch.tensor(3.0e4).to(dt))
        assert torch.isinf(inv[8]).all() and torch.isinf(amax[9]).all()


def test_empty_shapes(native, cuda):
    lib = L.load()
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.fp8mi_quantize_rowwise(None, L.BF16, 0, 128, 128, None, 128, None, None, E4, L.ENC_REFERENCE, stream) == 0
    q, inv = native.fp8_quantize_rowwise(torch.zeros(0, 64, dtype=torch.bfloat16, device=cuda))
    assert q.shape == (0, 64) and inv.shape == (0, 1)
    # cols == 0 with rows > 0: the scales are written, nothing else is touched
    for rows in (1, 5, 300):
        inv = torch.full((rows + 1,), 7.0, dtype=torch.float32, device=cuda)
        amax = torch.full((rows + 1,), 7.0, dtype=torch.float32, device=cuda)
        assert lib.fp8mi_quantize_rowwise(None, L.F32, rows, 0, 0, None, 0, inv.data_ptr(), amax.data_ptr(), E5, L.ENC_RNE, stream) == 0
        torch.cuda.synchronize()
        assert inv[:rows].eq(1.0).all() and amax[:rows].eq(0.0).all() and inv[rows].item() == 7.0 and amax[rows].item() == 7.0
    q, inv, amax = native.fp8_quantize_rowwise(torch.zeros(4, 0, device=cuda), return_amax=True)
    assert q.shape == (4, 0) and inv.view(-1).tolist() == [1.0] * 4 and amax.view(-1).tolist() == [0.0] * 4
    d = native.fp8_dequantize_rowwise(q, inv)
    assert d.shape == (4, 0) and d.dtype == torch.float32


def test_amax_output_given_and_null(cuda):
    rng = np.random.default_rng(51)
    for dt, rows, cols in ((torch.bfloat16, 9, 2048), (torch.float32, 3, 9000), (torch.float16, 2, 18000), (torch.float32, 7, 13)):
        x = make(rng, rows, cols, dt)
        xd = x.to(cuda)
        outs = []
        for with_amax in (True, False):
            out = torch.empty((rows, cols), dtype=torch.uint8, device=cuda)
            inv = torch.empty(rows, dtype=torch.float32, device=cuda)
            amax = torch.full((rows,), -3.0, dtype=torch.float32, device=cuda)
            raw_quantize(xd.data_ptr(), dt, rows, cols, cols, out.data_ptr(), cols, inv.data_ptr(), amax.data_ptr() if with_amax else None, E4, L.ENC_RNE)
            check_q(out, inv, amax if with_amax else None, x, E4, L.ENC_RNE, what=f"amax {with_amax} {rows}x{cols}")
            if not with_amax:
                assert amax.eq(-3.0).all()
            outs.append((out, inv))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ---------------------------------------------------------------------------------------------------------------------------
# quantiser against the existing per-tensor product code, row by row
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f16", "bf16"])
def test_rows_equal_the_per_tensor_quantisers(native, cuda, dt):
    rng = np.random.default_rng(61 + CODE[dt])
    for rows, cols in ((8, 3072), (5, 1000), (4, 14336), (3, 20000), (6, 37)):
        x = make(rng, rows, cols, dt)
        x[2, 1] = float("nan")
        x[1, 2], x[0, 0] = float("inf"), float("-inf")        # non-finite input behaves as in the per-tensor quantisers, row by row
        xd = x.to(cuda)
        for mode in (L.ENC_REFERENCE, L.ENC_RNE):
            q, inv = native.fp8_quantize_rowwise(xd, encode_mode=mode)
            for r in range(rows):
                wq, winv = native.fp8_quantize(xd[r], encode_mode=mode)
                assert torch.equal(q[r], wq), (rows, cols, mode, r)
                assert torch.equal(inv[r].view(torch.int32), winv.view(torch.int32)), (rows, cols, mode, r)
        q, inv = native.fp8_quantize_rowwise(xd, out_format=E5)
        for r in range(rows):
            wq, winv = native.fp8_quantize_e5m2(xd[r])
            assert torch.equal(q[r].view(torch.uint8), wq.view(torch.uint8)) and torch.equal(inv[r].view(torch.int32), winv.view(torch.int32)), (rows, cols, r)


# ---------------------------------------------------------------------------------------------------------------------------
# dequant
# ---------------------------------------------------------------------------------------------------------------------------

INT_OF = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}


def same_bits(got, want, what):
    got, want = got.cpu(), want.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, what
    gn, wn = torch.isnan(got), torch.isnan(want)
    assert torch.equal(gn, wn), (what, "NaN positions")
    gi, wi = got.view(INT_OF[got.dtype])[~gn], want.view(INT_OF[want.dtype])[~wn]
    bad = (gi != wi).nonzero().flatten()
    assert bad.numel() == 0, (what, bad[:8].tolist(), gi[bad[:8]].tolist(), wi[bad[:8]].tolist())


# per-row scales: plain, a subnormal fp32 product (2^-9 .. 448 times 2^-130), an fp32 overflow, a negative one, one that lands in
# float16's subnormals, one that overflows float16 / saturates nothing in bfloat16
DQ_SCALES = [1.0, 0.3, 2.0 ** -130, 1.0e38, -2.5, 2.0 ** -20, 1000.0, 1.0 / 3.0]


@pytest.mark.parametrize("fmt", [E4, E5], ids=["e4m3", "e5m2"])
@pytest.mark.parametrize("od", DTYPES, ids=["f32", "f16", "bf16"])
def test_dequant_all_256_bytes(native, cuda, od, fmt):
    rows = len(DQ_SCALES)
    q = np.tile(np.arange(256, dtype=np.uint8), (rows, 1))
    s = np.array(DQ_SCALES, np.float32)
    want = R.dequant_rowwise_ref(q, s, fmt, od)
    qd, sd = torch.from_numpy(q).to(cuda), torch.from_numpy(s).to(cuda)
    got = native.fp8_dequantize_rowwise(qd, sd, out_dtype=od, in_format=fmt)                  # streaming form (256 columns)
    same_bits(got, want, f"vector {od} {fmt}")
    typed = qd.view(torch.float8_e5m2 if fmt == E5 else torch.float8_e4m3fn)                  # the format from the dtype, (rows, 1) scales
    same_bits(native.fp8_dequantize_rowwise(typed, sd.reshape(rows, 1), out_dtype=od), want, f"typed {od} {fmt}")
    # ld_in > cols: slices of a wider buffer, with an aligned (320) and an odd (300) stride, and a column count that is no multiple of 16
    for ld, c0, cols in ((320, 0, 256), (300, 0, 256), (320, 16, 240), (320, 3, 100)):
        wide = torch.zeros((rows, ld), dtype=torch.uint8, device=cuda)
        wide[:, c0:c0 + cols] = qd[:, :cols]
        got = native.fp8_dequantize_rowwise(wide[:, c0:c0 + cols], sd, out_dtype=od, in_format=fmt)
        same_bits(got, want[:, :cols], f"ld {ld} c0 {c0} cols {cols} {od} {fmt}")
    # unaligned pointers through the C entry point: input at +1, output at +1 element
    lib = L.load()
    esz = torch.empty(0, dtype=od).element_size()
    for off_in, off_out in ((1, 0), (0, 1), (3, 1)):
        src = torch.zeros(rows * 256 + 16, dtype=torch.uint8, device=cuda)
        src[off_in:off_in + rows * 256] = qd.reshape(-1)
        dst = torch.zeros(rows * 256 + 8, dtype=od, device=cuda)
        rc = lib.fp8mi_dequant_rowwise(src.data_ptr() + off_in, rows, 256, 256, sd.data_ptr(), fmt, dst.data_ptr() + off_out * esz, CODE[od],
                                       torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        same_bits(dst[off_out:off_out + rows * 256].reshape(rows, 256), want, f"offsets {off_in} {off_out} {od} {fmt}")
        assert dst[:off_out].eq(0).all() and dst[off_out + rows * 256:].eq(0).all()


def test_quantize_dequantize_round_trip(native, cuda):
    rng = np.random.default_rng(71)
    x = make(rng, 64, 4096, torch.bfloat16)
    for fmt, mode in ((E4, L.ENC_REFERENCE), (E4, L.ENC_RNE), (E5, L.ENC_RNE)):
        q, inv = native.fp8_quantize_rowwise(x.to(cuda), out_format=fmt, encode_mode=mode)
        back = native.fp8_dequantize_rowwise(q, inv, out_dtype=torch.float32)
        wq, _, winv = R.quantize_rowwise_ref(x, fmt, mode)
        same_bits(back, R.dequant_rowwise_ref(wq, winv, fmt, torch.float32), f"round trip {fmt}")


# ---------------------------------------------------------------------------------------------------------------------------
# fp8_linear_rowwise
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wfmt", [E4, E5], ids=["w-e4m3", "w-e5m2"])
@pytest.mark.parametrize("per_channel", [False, True], ids=["ws1", "wsN"])
def test_linear_rowwise_is_the_gemm_on_the_reference_bytes(native, cuda, per_channel, wfmt):
    """fp8_linear_rowwise = one quantise launch + fp8_scaled_mm: with the reference's bytes and inverse scales as operands the same kernel
    runs on the same input, so the results are equal bit for bit."""
    rng = np.random.default_rng(81 + wfmt + 2 * per_channel)
    for (M, K, N), dt in (((4096, 3072, 3072), torch.bfloat16), ((64, 14336, 4096), torch.bfloat16), ((1, 4096, 1024), torch.float16),
                          ((37, 1000, 264), torch.float32)):
        x = make(rng, M, K, dt)
        w = torch.from_numpy((rng.standard_normal((N, K)) * 0.05 * np.exp2(rng.integers(-2, 3, size=(N, 1)))).astype(np.float32))
        bias = torch.from_numpy(rng.standard_normal(N).astype(np.float32)).to(cuda)
        if per_channel:
            wq, ws = native.fp8_quantize_rowwise(w.to(cuda), out_format=wfmt)
            ws = ws.reshape(-1)
            assert ws.numel() == N
        elif wfmt == E5:
            wq, ws = native.fp8_quantize_e5m2(w.to(cuda))
        else:
            wq, ws = native.fp8_quantize(w.to(cuda))
        y = native.fp8_linear_rowwise(x.to(cuda), wq, ws, bias)
        assert y.shape == (M, N) and y.dtype == dt
        rq, _, rinv = R.quantize_rowwise_ref(x, E4, native.ENCODE_MODE)
        want = native.fp8_scaled_mm(torch.from_numpy(rq).to(cuda), wq, torch.from_numpy(rinv).to(cuda).reshape(M, 1), ws, bias=bias, out_dtype=dt,
                                    b_format=wfmt)
        torch.cuda.synchronize()
        assert torch.equal(y.view(INT_OF[dt]), want.view(INT_OF[dt])), (M, K, N, dt)
    # leading dimensions are kept, the weight format may come as a keyword, out_dtype is honoured
    x3 = make(rng, 6, 512, torch.bfloat16).reshape(2, 3, 512)
    w = torch.from_numpy(rng.standard_normal((128, 512)).astype(np.float32) * 0.05)
    wq, ws = native.fp8_quantize_rowwise(w.to(cuda), out_format=wfmt)
    y = native.fp8_linear_rowwise(x3.to(cuda), wq.view(torch.uint8), ws, out_dtype=torch.float32, weight_format=wfmt)
    assert y.shape == (2, 3, 128) and y.dtype == torch.float32
    y2 = native.fp8_linear_rowwise(x3.to(cuda).reshape(6, 512), wq, ws, out_dtype=torch.float32)
    assert torch.equal(y.reshape(6, 128), y2)


# ---------------------------------------------------------------------------------------------------------------------------
# the torch._scaled_mm route on the quantiser's outputs
# ---------------------------------------------------------------------------------------------------------------------------

def test_scaled_mm_patch_on_rowwise_outputs(cuda, patch, native):
    rng = np.random.default_rng(91)
    f8 = torch.float8_e4m3fn
    for M, K, N in ((256, 3072, 512), (64, 4096, 1024), (33, 1024, 136)):
        x = make(rng, M, K, torch.bfloat16)
        w = make(rng, N, K, torch.bfloat16)
        q, inv = native.fp8_quantize_rowwise(x.to(cuda))
        wq, winv = native.fp8_quantize_rowwise(w.to(cuda))
        assert inv.shape == (M, 1) and winv.t().shape == (1, N)
        got = torch._scaled_mm(q.view(f8), wq.view(f8).t(), scale_a=inv, scale_b=winv.t(), out_dtype=torch.bfloat16)
        want = native.fp8_scaled_mm(q, wq, inv, winv, out_dtype=torch.bfloat16, nan_mode=native.NAN_MODE)
        torch.cuda.synchronize()
        assert got.dtype == torch.bfloat16 and torch.equal(got.view(torch.int16), want.view(torch.int16)), (M, K, N)
        assert torch.isfinite(got).all()


# ---------------------------------------------------------------------------------------------------------------------------
# graph capture
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,cols", [(128, 3072), (16, 14336), (4, 20000)], ids=["wave-per-row", "workgroup-per-row", "looping"])
def test_quantize_launch_replays_in_a_graph(native, cuda, rows, cols):
    """One kernel launch, no workspace, no host sync: captured once, replayed on new data.  (A single kernel node: no parallel branches.)"""
    rng = np.random.default_rng(rows + cols)
    xs = make(rng, rows, cols, torch.bfloat16).to(cuda)
    native.fp8_quantize_rowwise(xs, encode_mode=L.ENC_RNE, return_amax=True)      # warm-up: the library is loaded, the allocator primed
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        q, inv, amax = native.fp8_quantize_rowwise(xs, encode_mode=L.ENC_RNE, return_amax=True)
    for _ in range(2):
        x = make(rng, rows, cols, torch.bfloat16)
        xs.copy_(x.to(cuda))
        g.replay()
        torch.cuda.synchronize()
        check_q(q, inv, amax, x, E4, L.ENC_RNE, what=f"graph replay {rows}x{cols}")


# ---------------------------------------------------------------------------------------------------------------------------
# C ABI from a plain C host
# ---------------------------------------------------------------------------------------------------------------------------

def test_c_abi_rowwise_roundtrip_without_torch(cuda, tmp_path):
    exe = str(tmp_path / "rowwise_roundtrip")
    cmd = ["gcc", "-O2", "-D__HIP_PLATFORM_AMD__", os.path.join(ROOT, "tests", "c", "rowwise_roundtrip.c"), "-I/opt/rocm/include",
           "-I" + os.path.join(ROOT, "include"), "-L" + PKG, "-lfp8mi", "-L/opt/rocm/lib", "-lamdhip64", "-lm",
           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "rowwise C ABI round trip: ok" in out.stdout
