"""GPU: the fused normalisation + quantisation launch (fp8mi_norm_quantize / fp8_norm_quantize) and the linears built on it, against
tests/norm_quant_ref.py.

Every call asks for mean_out / rstd_out.  The returned statistics are held to caps against float64 (norm_quant_ref.stat_ratios:
2^-18 of mean|h| for the mean, 2^-18 relative for rstd; tests/test_norm_quant_host.py checks on the CPU that lane-ordered float32 sums
of these very inputs stay within a quarter of them).  With those statistics fed to the reference, the bytes, the scales and amax are
compared byte for byte and bit for bit: no tolerance, for every variant - what one rounding per operation buys.

Rows whose y holds NaNs (test_special_rows) are compared exactly too - a generated NaN (inf * 0) as the reference pins it, a NaN that came
from one operand with that operand's sign - except where two NaNs meet in one operation, a NaN element times a NaN statistic: the result's
sign is not specified there (include/fp8mi.h), the RNE / e5m2 row encoders copy it, and those bytes alone are compared without it."""
import numpy as np
import pytest
import torch

import fp8_mi355x_lib as L
import norm_quant_ref as NR

pytestmark = pytest.mark.gpu

E4, E5 = L.FMT_E4M3, L.FMT_E5M2
CODE = {torch.float32: L.F32, torch.float16: L.F16, torch.bfloat16: L.BF16}
NORM = {"rms": L.NORM_RMS, "layer": L.NORM_LAYER}
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
DT_IDS = ["f32", "f16", "bf16"]
# (scale, out_format, encode_mode): the four combinations of tests/test_gpu_act_quant.py
QS = [("row", E4, L.ENC_REFERENCE), ("row", E4, L.ENC_RNE), ("row", E5, L.ENC_RNE), ("block128", E4, L.ENC_RNE)]
QS_IDS = ["row-e4m3-reference", "row-e4m3-rne", "row-e5m2", "block128"]
INT_OF = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}
VARIANTS = ["plain", "weight", "weight_bias", "mod", "residual", "all"]
EPS = 1e-6

COLS = [1, 2, 7, 8, 100, 128, 129, 200, 1024, 3072, 4100, 8192, 16384, 16400]
ROWS = [1, 3, 5, 257]


def seed(norm, dt, cols, rows):
    return 100000 * NORM[norm] + 10000 * CODE[dt] + 7 * cols + rows


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(INT_OF[a.dtype]), b.contiguous().view(INT_OF[b.dtype]))


def check_exact(q, sc, amax, want, what="", nan_y=None):
    """device q / sc / amax (amax may be None) against the reference triple, byte for byte and bit for bit; nan_y: the elements whose y is
    a NaN - their bytes are compared without the sign bit"""
    wq, ws, wamax = want
    g = q.view(torch.uint8).cpu().numpy().reshape(wq.shape)
    if nan_y is not None:
        g, wq = np.where(nan_y, g & 0x7F, g), np.where(nan_y, wq & 0x7F, wq)
    bad = np.argwhere(g != wq)
    assert bad.shape[0] == 0, (what, bad.shape[0], [(int(r), int(c), hex(int(g[r, c])), hex(int(wq[r, c]))) for r, c in bad[:6]])
    gs = sc.cpu().numpy().reshape(ws.shape)
    assert np.array_equal(bits(gs), bits(ws)), (what, "scales", gs.reshape(-1)[:4], ws.reshape(-1)[:4])
    if amax is not None:
        assert np.array_equal(bits(amax.cpu().numpy().reshape(-1)), bits(wamax)), (what, "amax")


def variant_inputs(rng, variant, rows, cols, dt, pdt, rows_per_mod=2):
    """-> the keyword arguments (CPU tensors) of a variant: weight / bias / mod_scale / mod_shift of dtype pdt, residual of dtype dt"""
    kw = {}
    if variant in ("weight", "weight_bias", "all"):
        kw["weight"] = NR.make_params(rng, 1, cols, pdt, 1.0)[0]
    if variant in ("weight_bias", "all"):
        kw["bias"] = NR.make_params(rng, 1, cols, pdt)[0]
    if variant in ("mod", "all"):
        nmod = -(-rows // rows_per_mod)
        kw["mod_scale"], kw["mod_shift"], kw["rows_per_mod"] = NR.make_params(rng, nmod, cols, pdt), NR.make_params(rng, nmod, cols, pdt), rows_per_mod
    if variant in ("residual", "all"):
        kw["residual"] = NR.make_rows(rng, rows, cols, dt)
    return kw


def ptr(t):
    return None if t is None else t.data_ptr()


def raw(cuda, x, norm, scale, fmt, mode, eps=EPS, weight=None, bias=None, mod_scale=None, mod_shift=None, rows_per_mod=1, residual=None, h_alias=False):
    """The C entry point on contiguous device copies of CPU tensors -> dict of device results (q, sc, amax, mean, rstd, h)"""
    rows, cols = x.shape
    dev = lambda t: None if t is None else t.to(cuda).contiguous()   # noqa: E731
    xd, w, b, msc, msh, res = dev(x), dev(weight), dev(bias), dev(mod_scale), dev(mod_shift), dev(residual)
    params = [t for t in (w, b, msc, msh) if t is not None]
    pdt = params[0].dtype if params else x.dtype
    row = scale == "row"
    ncb = 1 if row else -(-cols // 128)
    q = torch.empty((rows, cols), dtype=torch.uint8, device=cuda)
    sc = torch.empty((rows, ncb), dtype=torch.float32, device=cuda)
    amax = torch.empty(rows, dtype=torch.float32, device=cuda) if row else None
    layer = norm == "layer"
    mean = torch.full((rows,), 7.0, dtype=torch.float32, device=cuda) if layer else None
    rstd = torch.full((rows,), 7.0, dtype=torch.float32, device=cuda)
    h = None if res is None else (res if h_alias else torch.empty_like(res))
    ld = max(cols, 1)
    rc = L.load().fp8mi_norm_quantize(xd.data_ptr(), CODE[x.dtype], rows, cols, ld, NORM[norm], eps, ptr(w), ptr(b), ptr(msc), ptr(msh), ld, rows_per_mod,
                                      CODE[pdt], ptr(res), ld, ptr(h), ld, q.data_ptr(), ld, sc.data_ptr(), ncb, 1, ptr(amax),
                                      L.QSCALE_ROW if row else L.QSCALE_GROUP128, fmt, mode, ptr(mean), rstd.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.load().fp8mi_last_error()
    torch.cuda.synchronize()
    return dict(q=q, sc=sc, amax=amax, mean=mean, rstd=rstd, h=h)


def verify(got, x, norm, scale, fmt, mode, what, eps=EPS, masked=False, **kw):
    """statistics within their caps; then bytes, scales, amax (and h) exact against the reference fed with the returned statistics"""
    h_ref, stored = NR.norm_h(x, kw.get("residual"))
    mean = None if got["mean"] is None else got["mean"].cpu().numpy()
    rstd = got["rstd"].cpu().numpy()
    if x.shape[1]:
        mr, rr = NR.stat_ratios(h_ref, norm, eps, mean, rstd)
        print(f"[norm_quant] {what}: mean at {mr:.3f} of its cap, rstd at {rr:.3f}")
        assert mr <= 1.0 and rr <= 1.0, (what, "statistics", mr, rr)
    want, y, _ = NR.norm_quantize_ref(x, norm, eps=eps, scale=scale, fmt=fmt, mode=mode, mean=mean, rstd=rstd, **kw)
    # masked: the sign bit of a NaN byte is set aside where two NaNs met - and only there, and only under the encoders that copy it
    loose = NR.two_nan_elements(x, norm, kw.get("residual"), mean, rstd) if masked and scale == "row" and mode != L.ENC_REFERENCE else None
    check_exact(got["q"], got["sc"], got["amax"], want, what, nan_y=loose)
    if stored is not None:
        assert same(got["h"].cpu(), stored), (what, "h_out")
    return y


def run_grid(cuda, dt, norm, qs_index, variant_of, pdt_of):
    scale, fmt, mode = QS[qs_index]
    for ci, cols in enumerate(COLS):
        for ri, rows in enumerate(ROWS):
            rng = np.random.default_rng(seed(norm, dt, cols, rows))
            x = NR.make_rows(rng, rows, cols, dt, norm == "layer")          # the first draw: what the host test checks the caps on
            variant, pdt = variant_of(ci, ri), pdt_of(ci, ri)
            kw = variant_inputs(rng, variant, rows, cols, dt, pdt)
            got = raw(cuda, x, norm, scale, fmt, mode, **kw)
            verify(got, x, norm, scale, fmt, mode, f"{norm} {dt} {variant} params {pdt} {QS_IDS[qs_index]} {rows}x{cols}", **kw)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the grid: every form, every variant
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("qs_index", range(4), ids=QS_IDS)
@pytest.mark.parametrize("norm", ["rms", "layer"])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_grid_variants_spread(cuda, dt, norm, qs_index):
    """Register-resident with one wave per row and with several, looping (16400), any alignment (1, 2, 7, 129, ... columns), whole and
    partial groups.  The six variants rotate over columns and rows, shifted by dtype, norm and recipe, so that each meets every form;
    the parameters of 16-bit input are fp32 in every other cell."""
    off = CODE[dt] + 2 * qs_index + NORM[norm]
    run_grid(cuda, dt, norm, qs_index, lambda ci, ri: VARIANTS[(ci + ri + off) % 6],
             lambda ci, ri: torch.float32 if (ci + ri + qs_index) % 2 else dt)


@pytest.mark.parametrize("qs_index", range(4), ids=QS_IDS)
@pytest.mark.parametrize("norm", ["rms", "layer"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_grid_bf16_every_variant(cuda, variant, norm, qs_index):
    run_grid(cuda, torch.bfloat16, norm, qs_index, lambda ci, ri: variant, lambda ci, ri: torch.bfloat16 if (ci + ri) % 3 else torch.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. layout edges through the C entry point
# ---------------------------------------------------------------------------------------------------------------------------

def padded(cuda, t, ld, fill):
    """t (rows, cols) inside a (rows, ld) device buffer filled with `fill`; -> (buffer, view)"""
    buf = torch.full((t.shape[0], ld), fill, dtype=t.dtype, device=cuda)
    buf[:, :t.shape[1]] = t.to(cuda)
    return buf, buf[:, :t.shape[1]]


@pytest.mark.parametrize("scale,fmt,mode", [QS[0], QS[2], QS[3]], ids=[QS_IDS[0], QS_IDS[2], QS_IDS[3]])
@pytest.mark.parametrize("norm", ["rms", "layer"])
def test_leading_dimensions_scale_strides_and_untouched_padding(cuda, norm, scale, fmt, mode):
    """Every leading dimension larger than the row - aligned (vector forms) and odd (any-alignment form) - with the inputs inside
    NaN-filled buffers and the outputs inside 0xA5- / NaN-filled ones: nothing outside the result is written.  Scales row-major and
    outer-dim-major.  rows_per_mod of 1, 3 and rows, rows not a multiple of it."""
    rng = np.random.default_rng(11 + NORM[norm] + fmt + mode)
    smode = L.QSCALE_ROW if scale == "row" else L.QSCALE_GROUP128
    nan = float("nan")
    dts = {0: torch.bfloat16, 1: torch.float32, 2: torch.float16}
    # (rows, cols, pads of ld_in, ld_res, ld_h, ld_mod, ld_out, rows_per_mod)
    cases = ((37, 1000, (24, 8, 16, 40, 8), 3), (37, 1000, (1, 3, 5, 7, 3), 1), (5, 3072, (1024, 0, 8, 0, 0), 5), (7, 8192, (0, 16, 0, 8, 16), 3),
             (3, 20000, (480, 16, 32, 8, 16), 1), (2, 20000, (1, 1, 3, 1, 0), 3), (9, 16, (0, 1, 0, 0, 1), 9), (4, 12288, (8, 8, 8, 8, 16), 3))
    for i, (rows, cols, (p_in, p_res, p_h, p_mod, p_out), rpm) in enumerate(cases):
        dt = dts[i % 3]
        pdt = dt if i % 2 else torch.float32
        x = NR.make_rows(rng, rows, cols, dt, norm == "layer")
        kw = variant_inputs(rng, "all", rows, cols, dt, pdt, rows_per_mod=rpm)
        xb, _ = padded(cuda, x, cols + p_in, nan)
        rb, _ = padded(cuda, kw["residual"], cols + p_res, nan)
        mscb, _ = padded(cuda, kw["mod_scale"], cols + p_mod, nan)
        mshb, _ = padded(cuda, kw["mod_shift"], cols + p_mod, nan)
        w, b = kw["weight"].to(cuda), kw["bias"].to(cuda)
        ld_out, ld_h = cols + p_out, cols + p_h
        ncb = -(-cols // 128) if scale == "block128" else 1
        for outer_major in (False, True):
            out = torch.full((rows * ld_out + 64,), 0xA5, dtype=torch.uint8, device=cuda)
            hb = torch.full((rows, ld_h), nan, dtype=dt, device=cuda)
            sc = torch.full((rows * ncb + 8,), nan, dtype=torch.float32, device=cuda)
            amax = torch.empty(rows, dtype=torch.float32, device=cuda) if scale == "row" else None
            stats = torch.full((2, rows + 1), 7.0, dtype=torch.float32, device=cuda)
            layer = norm == "layer"
            s_sr, s_sk = (1, rows) if outer_major else (ncb, 1)
            rc = L.load().fp8mi_norm_quantize(xb.data_ptr(), CODE[dt], rows, cols, cols + p_in, NORM[norm], EPS, w.data_ptr(), b.data_ptr(), mscb.data_ptr(),
                                              mshb.data_ptr(), cols + p_mod, rpm, CODE[pdt], rb.data_ptr(), cols + p_res, hb.data_ptr(), ld_h,
                                              out.data_ptr(), ld_out, sc.data_ptr(), s_sr, s_sk, ptr(amax), smode, fmt, mode,
                                              stats[0].data_ptr() if layer else None, stats[1].data_ptr(), torch.cuda.current_stream().cuda_stream)
            assert rc == 0, L.load().fp8mi_last_error()
            torch.cuda.synchronize()
            what = f"{norm} {rows}x{cols} {dt} params {pdt} pads {(p_in, p_res, p_h, p_mod, p_out)} rows_per_mod {rpm} outer-major {outer_major}"
            o2 = out[:rows * ld_out].reshape(rows, ld_out)
            got_s = sc[:rows * ncb].reshape(ncb, rows).t() if outer_major else sc[:rows * ncb].reshape(rows, ncb)
            got = dict(q=o2[:, :cols].contiguous(), sc=got_s.contiguous(), amax=amax, mean=stats[0, :rows] if layer else None, rstd=stats[1, :rows],
                       h=hb[:, :cols].contiguous())
            verify(got, x, norm, scale, fmt, mode, what, **kw)
            assert o2[:, cols:].eq(0xA5).all() and out[rows * ld_out:].eq(0xA5).all(), (what, "padding bytes written")
            assert torch.isnan(sc[rows * ncb:]).all(), (what, "scales written past the end")
            assert torch.isnan(hb[:, cols:]).all(), (what, "h_out written past the row")
            assert stats[:, rows].eq(7.0).all() and (layer or stats[0].eq(7.0).all()), (what, "statistics written past the end")


@pytest.mark.parametrize("scale,fmt,mode", [QS[1], QS[3]], ids=[QS_IDS[1], QS_IDS[3]])
@pytest.mark.parametrize("norm", ["rms", "layer"])
def test_h_out_may_be_the_residual(cuda, norm, scale, fmt, mode):
    """In-place stream update on the register-resident forms, the looping form (20000 columns) and the any-alignment form."""
    rng = np.random.default_rng(61 + NORM[norm] + fmt + mode)
    for dt, rows, cols in ((torch.bfloat16, 9, 3072), (torch.float16, 5, 8192), (torch.float32, 3, 16384), (torch.bfloat16, 3, 20000),
                           (torch.float32, 4, 20000), (torch.bfloat16, 6, 4100), (torch.float16, 7, 129)):
        x = NR.make_rows(rng, rows, cols, dt, norm == "layer")
        kw = variant_inputs(rng, "all", rows, cols, dt, dt, rows_per_mod=2)
        got = raw(cuda, x, norm, scale, fmt, mode, h_alias=True, **kw)
        verify(got, x, norm, scale, fmt, mode, f"aliased {norm} {dt} {rows}x{cols}", **kw)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the residual identity, on the device
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scale,fmt,mode", QS, ids=QS_IDS)
@pytest.mark.parametrize("norm", ["rms", "layer"])
def test_residual_call_is_torchs_sum_then_the_plain_call(native, cuda, norm, scale, fmt, mode):
    rng = np.random.default_rng(71 + NORM[norm] + fmt + mode)
    for dt, rows, cols in ((torch.bfloat16, 33, 3072), (torch.float16, 5, 8192), (torch.float32, 3, 16384), (torch.bfloat16, 3, 16400),
                           (torch.float16, 6, 4100), (torch.float32, 7, 129), (torch.bfloat16, 257, 200)):
        x, res = NR.make_rows(rng, rows, cols, dt, norm == "layer").to(cuda), NR.make_rows(rng, rows, cols, dt).to(cuda)
        w = NR.make_params(rng, 1, cols, dt, 1.0)[0].to(cuda)
        kw = dict(norm=norm, weight=w, scale=scale, out_format=fmt, encode_mode=mode, return_stats=True)
        fused = native.fp8_norm_quantize(x, residual=res, **kw)
        summed = x + res
        plain = native.fp8_norm_quantize(summed, **kw)
        assert same(fused[2], summed), (dt, rows, cols, "h")
        assert torch.equal(fused[0].view(torch.uint8), plain[0].view(torch.uint8)) and same(fused[1], plain[1]), (dt, rows, cols)
        assert all(same(a, b) for a, b in zip(fused[3:], plain[2:])), (dt, rows, cols, "statistics")


# ---------------------------------------------------------------------------------------------------------------------------
# 4. special rows
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scale,fmt,mode", QS, ids=QS_IDS)
@pytest.mark.parametrize("norm", ["rms", "layer"])
def test_special_rows(cuda, norm, scale, fmt, mode):
    """An all-zero row (rstd = 1 / sqrt(eps), y = bias / shift; eps = 0: NaN bytes), a row holding a NaN, +inf, -inf, both infinities: plain
    IEEE arithmetic, compared with the reference fed with the returned statistics (the sign of a NaN byte set aside only where two NaNs met)."""
    rng = np.random.default_rng(81 + NORM[norm] + fmt + mode)
    inf, nan = float("inf"), float("nan")
    for dt, cols in ((torch.float32, 776), (torch.bfloat16, 3072), (torch.float16, 8192), (torch.bfloat16, 20000), (torch.float32, 50), (torch.float16, 129)):
        x = NR.make_rows(rng, 8, cols, dt, norm == "layer")
        x[1] = 0.0
        x[2, cols // 3] = nan
        x[3, cols - 1] = inf
        x[4, 0], x[4, cols // 2] = inf, -inf
        x[5, 1] = -inf
        x[6, 0], x[6, 1] = nan, inf
        for variant in ("plain", "weight_bias", "mod"):
            kw = variant_inputs(rng, variant, 8, cols, dt, dt, rows_per_mod=3)
            for eps in (EPS, 0.0):
                got = raw(cuda, x, norm, scale, fmt, mode, eps=eps, **kw)
                y = verify(got, x, norm, scale, fmt, mode, f"specials {norm} {dt} {cols} {variant} eps {eps}", eps=eps, masked=True, **kw)
                rstd, g = got["rstd"].cpu().numpy(), got["q"].cpu().numpy()
                assert np.isnan(rstd[[2, 6]]).all() and np.isnan(y[[2, 6]]).all() and np.isfinite(rstd[[0, 7]]).all(), (dt, cols, rstd)
                assert ((g[[2, 6]] & 0x7F) == 0x7F).all()
                if norm == "rms":      # the sum of squares is inf, rstd = 0: finite elements give 0 (before bias / shift), the infinite ones NaN
                    assert (rstd[[3, 4, 5]] == 0.0).all() and np.isnan(y[3, cols - 1]) and np.isnan(y[5, 1]) and np.isnan(y[4, [0, cols // 2]]).all()
                    assert np.isfinite(y[3, :cols - 1]).all() and np.isfinite(y[4, 1:cols // 2]).all()
                else:                  # the mean is inf (NaN for both signs), d is -inf or NaN: everything is NaN
                    assert np.isnan(rstd[[3, 4, 5]]).all() and np.isinf(got["mean"].cpu().numpy()[[3, 5]]).all() and np.isnan(y[[3, 4, 5]]).all()
                    assert ((g[[3, 4, 5]] & 0x7F) == 0x7F).all()
                if eps == 0.0:
                    assert np.isinf(rstd[1]) and np.isnan(y[1]).all() and ((g[1] & 0x7F) == 0x7F).all()
                else:
                    assert bits(rstd[1:2])[0] == bits(np.float32(1.0) / np.sqrt(np.float32(eps)))[0]
                    if variant == "plain":
                        assert (y[1] == 0).all() and (g[1] & 0x7F == 0).all()
                    elif variant == "weight_bias":
                        assert np.array_equal(bits(y[1]), bits(NR.widen(kw["bias"])))
                    else:
                        assert np.array_equal(y[1], NR.widen(kw["mod_shift"])[0])     # 0 * (1 + sc) + sh
    # empty shapes: rows == 0 is a no-op; cols == 0 writes the ROW scales (1) and amax (0) and no statistics
    lib, stream = L.load(), torch.cuda.current_stream().cuda_stream
    smode = L.QSCALE_ROW if scale == "row" else L.QSCALE_GROUP128
    assert lib.fp8mi_norm_quantize(None, L.BF16, 0, 128, 128, NORM[norm], EPS, None, None, None, None, 128, 1, L.BF16, None, 128, None, 128, None, 128, None, 1, 1,
                                   None, smode, fmt, mode, None, None, stream) == 0
    for rows in (1, 5, 300):
        buf = torch.full((4, rows + 1), 7.0, dtype=torch.float32, device=cuda)
        row = scale == "row"
        assert lib.fp8mi_norm_quantize(None, L.F32, rows, 0, 0, NORM[norm], EPS, None, None, None, None, 0, 1, L.F32, None, 0, None, 0, None, 0,
                                       buf[0].data_ptr(), 1, 1, buf[1].data_ptr() if row else None, smode, fmt, mode,
                                       buf[2].data_ptr() if norm == "layer" else None, buf[3].data_ptr(), stream) == 0
        torch.cuda.synchronize()
        if row:
            assert buf[0, :rows].eq(1.0).all() and buf[1, :rows].eq(0.0).all()
        assert buf[2:].eq(7.0).all() and buf[:, rows].eq(7.0).all() and (row or buf.eq(7.0).all())


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the op layer
# ---------------------------------------------------------------------------------------------------------------------------

def test_three_d_input_with_per_image_modulation_and_column_slices(native, cuda):
    rng = np.random.default_rng(91)
    B, T, C = 3, 50, 3072
    x = NR.make_rows(rng, B * T, C, torch.bfloat16, True)
    sc, sh = NR.make_params(rng, B, C, torch.bfloat16), NR.make_params(rng, B, C, torch.bfloat16)
    for scale, fmt, mode in QS:
        for msc, msh in ((sc, sh), (sc.reshape(B, 1, C), sh.reshape(B, 1, C))):
            q, s, rstd, mean = native.fp8_norm_quantize(x.reshape(B, T, C).to(cuda), "layer", mod_scale=msc.to(cuda), mod_shift=msh.to(cuda), scale=scale,
                                                        out_format=fmt, encode_mode=mode, return_stats=True)
            assert q.shape == (B, T, C) and s.shape == (B, T, 1 if scale == "row" else C // 128) and rstd.shape == mean.shape == (B, T, 1)
            assert q.dtype == (torch.float8_e5m2 if fmt == E5 else torch.uint8)
            got = dict(q=q.reshape(B * T, C), sc=s.reshape(B * T, -1), amax=None, mean=mean.reshape(-1), rstd=rstd.reshape(-1), h=None)
            verify(got, x, "layer", scale, fmt, mode, f"3-D adaLN {scale}", mod_scale=sc, mod_shift=sh, rows_per_mod=T)
    # column slices of a wider tensor are read in place (x and the residual alike); the module's default encode mode
    wide, rwide = NR.make_rows(rng, 40, 4096, torch.bfloat16), NR.make_rows(rng, 40, 4096, torch.bfloat16)
    wd, rd = wide.to(cuda), rwide.to(cuda)
    for c0, width in ((512, 3072), (8, 1024), (3, 100), (1, 4094)):
        w = NR.make_params(rng, 1, width, torch.float32, 1.0)[0]
        r0 = c0 + 8 if c0 + 8 + width <= 4096 else 0
        xs, rs, rview = wide[:, c0:c0 + width].contiguous(), rwide[:, r0:r0 + width].contiguous(), rd[:, r0:r0 + width]
        q, s, h, rstd = native.fp8_norm_quantize(wd[:, c0:c0 + width], "rms", weight=w.to(cuda), residual=rview, return_stats=True)
        assert q.is_contiguous() and h.is_contiguous() and h.dtype == torch.bfloat16
        got = dict(q=q, sc=s, amax=None, mean=None, rstd=rstd.reshape(-1), h=h)
        verify(got, xs, "rms", "row", E4, native.ENCODE_MODE, f"slice {c0}+{width}", weight=w, residual=rs)
    with pytest.raises(L.Fp8miError):
        native.fp8_norm_quantize(wd, out_format=E5, encode_mode=L.ENC_REFERENCE)


# Relative rms error of an FP8 linear against the float32 chain.  tests/test_gpu_act_quant.py prints this distance for fp8_mlp_* and
# asserts no number, so the bound is derived here: an e4m3 operand element carries a relative rounding error of at most 2^-4 (three
# mantissa bits; elements in the subnormal range of their row's scale are below 2^-6 / 448 of the row's largest and do not weigh), so a
# product of two carries at most 2^-4 + 2^-4 + 2^-8, and sums of products whose errors are not all aligned stay below that: 2^-3.
LINEAR_REL_RMS = 2.0 ** -3


@pytest.mark.parametrize("recipe", ["rowwise", "blockwise"])
def test_norm_linears_are_their_two_steps(native, cuda, recipe):
    N_ = native
    F = torch.nn.functional
    rng = np.random.default_rng(95 + (recipe == "blockwise"))
    for (B, T, K, Nn), dt, norm in (((2, 35, 256, 200), torch.bfloat16, "layer"), ((1, 1, 512, 64), torch.float16, "rms"), ((3, 13, 384, 136), torch.float32, "rms"),
                                    ((2, 64, 3072, 256), torch.bfloat16, "layer")):
        x = NR.make_rows(rng, B * T, K, dt, norm == "layer").reshape(B, T, K).to(cuda)
        res = NR.make_rows(rng, B * T, K, dt).reshape(B, T, K).to(cuda)
        w = torch.from_numpy((rng.standard_normal((Nn, K)) / np.sqrt(K)).astype(np.float32)).to(cuda)
        bias = torch.from_numpy(rng.standard_normal(Nn).astype(np.float32) * 0.1).to(cuda)
        nw, nb = NR.make_params(rng, 1, K, dt, 1.0)[0].to(cuda), NR.make_params(rng, 1, K, dt)[0].to(cuda)
        sc, sh = NR.make_params(rng, B, K, dt).to(cuda), NR.make_params(rng, B, K, dt).to(cuda)
        kw = dict(norm=norm, weight=nw, norm_bias=nb, eps=1e-5, mod_scale=sc, mod_shift=sh)
        qkw = dict(norm=norm, weight=nw, bias=nb, eps=1e-5, mod_scale=sc, mod_shift=sh)
        if recipe == "rowwise":
            wq, ws = N_.fp8_quantize_rowwise(w)
            lin = lambda **k: N_.fp8_norm_linear_rowwise(x, wq, ws, bias=bias, **kw, **k)                                      # noqa: E731
            mm = lambda q, s, od: N_.fp8_scaled_mm(q.reshape(-1, K), wq, s.reshape(-1, 1), ws, bias=bias, out_dtype=od)       # noqa: E731
            scale, wd = "row", N_.fp8_dequantize_rowwise(wq, ws)
        else:
            wq, ws = N_.fp8_quantize_blockwise(w, 128)
            lin = lambda **k: N_.fp8_norm_linear_blockwise(x, wq, ws, bias=bias, **kw, **k)                                    # noqa: E731
            mm = lambda q, s, od: N_.fp8_scaled_mm_blockwise(q.reshape(-1, K), wq, s.reshape(B * T, -1), ws, block_a=1, block_b=128, bias=bias,   # noqa: E731
                                                             out_dtype=od)
            scale, wd = "block128", N_.fp8_dequantize_blockwise(wq, ws, 128)
        y = lin()
        assert y.shape == (B, T, Nn) and y.dtype == dt
        q, s = N_.fp8_norm_quantize(x, scale=scale, **qkw)
        assert same(y.reshape(B * T, Nn), mm(q, s, dt)), (recipe, dt, "two public steps")
        y2, h = lin(residual=res, out_dtype=torch.float32)
        q, s, h2 = N_.fp8_norm_quantize(x, residual=res, scale=scale, **qkw)
        assert y2.dtype == torch.float32 and same(h, x + res) and same(h, h2) and same(y2.reshape(B * T, Nn), mm(q, s, torch.float32)), (recipe, dt, "residual")
        # against the float32 torch chain on the dequantised weight
        hf = (x + res).float()
        n = F.layer_norm(hf, (K,), nw.float(), nb.float(), 1e-5) if norm == "layer" else F.rms_norm(hf, (K,), nw.float(), 1e-5) + nb.float()
        n = n * (1.0 + sc.float()[:, None, :]) + sh.float()[:, None, :]
        want = (n.reshape(-1, K) @ wd.float().t() + bias).double()
        rel = float(((y2.reshape(B * T, Nn).double() - want) ** 2).mean().sqrt() / (want ** 2).mean().sqrt())
        print(f"[norm_quant linear] {recipe} {norm} {(B, T, K, Nn)} {dt}: relative rms error against the float32 chain {rel:.4f}")
        assert rel <= LINEAR_REL_RMS, (recipe, dt, rel)


@pytest.mark.parametrize("norm,scale", [("layer", "row"), ("rms", "block128"), ("rms", "row")], ids=["layer-row", "rms-block128", "rms-row"])
@pytest.mark.parametrize("rows,cols", [(128, 3072), (16, 14336), (4, 20000)], ids=["wave-per-row", "workgroup-per-row", "looping"])
def test_launch_replays_in_a_graph(native, cuda, rows, cols, norm, scale):
    """Captured once, replayed twice on new data: the same bytes as the reference; an eager call is one launch."""
    rng = np.random.default_rng(rows + cols)
    layer = norm == "layer"
    xs, rs = NR.make_rows(rng, rows, cols, torch.bfloat16, layer).to(cuda), NR.make_rows(rng, rows, cols, torch.bfloat16).to(cuda)
    w = NR.make_params(rng, 1, cols, torch.bfloat16, 1.0)[0]
    wd = w.to(cuda)
    call = lambda: native.fp8_norm_quantize(xs, norm, weight=wd, residual=rs, scale=scale, encode_mode=L.ENC_RNE, return_stats=True)   # noqa: E731
    with L.kernel_timer(8) as prof:
        call()
    torch.cuda.synchronize()
    assert len(prof.ms) == 1, "one launch"
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    for _ in range(2):
        x, r = NR.make_rows(rng, rows, cols, torch.bfloat16, layer), NR.make_rows(rng, rows, cols, torch.bfloat16)
        xs.copy_(x.to(cuda))
        rs.copy_(r.to(cuda))
        g.replay()
        torch.cuda.synchronize()
        got = dict(q=out[0], sc=out[1], amax=None, h=out[2], rstd=out[3].reshape(-1), mean=out[4].reshape(-1) if layer else None)
        verify(got, x, norm, scale, E4, L.ENC_RNE, f"graph replay {norm} {rows}x{cols}", weight=w, residual=r)
