"""GPU: the fused producers with MXFP8 / MXFP4 output (fp8mi_act_quantize_mx / fp8mi_norm_quantize_mx; fp8_act_quantize and
fp8_norm_quantize with scale="mxfp8" | "mxfp4") and the MLPs / norm-linears built on them, against tests/mx_fused_ref.py.

act="none" and every normalisation variant (the reference fed with the statistics the GPU returned) are compared byte for byte, element
bytes and scale bytes: no tolerance.  The transcendental activations are held to the conditions of mx_fused_ref.compare_transcendental
against the float64-derived reference: every block's scale byte is the reference's, except that a block whose descale lies within 2^-18
relative of a power of two may take either neighbour of that power; element codes are compared with the recipe evaluated with the GPU's
exponent and may be one step off in at most 1e-3 of a tensor's elements; the excused blocks are at most max(1, 2 %) of a tensor's blocks
(tests/test_mx_fused_host.py checks on the CPU that the inputs leave that room)."""
import numpy as np
import pytest
import torch

import fp8_mi355x_lib as L
import mx_fused_ref as MX
import norm_quant_ref as NR

pytestmark = pytest.mark.gpu

CODE = {torch.float32: L.F32, torch.float16: L.F16, torch.bfloat16: L.BF16}
ACT = {"none": L.ACT_NONE, "silu": L.ACT_SILU, "gelu_tanh": L.ACT_GELU_TANH, "gelu_erf": L.ACT_GELU_ERF}
NORM = {"rms": L.NORM_RMS, "layer": L.NORM_LAYER}
FMT = {"mxfp8": L.MX_FP8, "mxfp4": L.MX_FP4}
DTYPES = [torch.float32, torch.float16, torch.bfloat16]
DT_IDS = ["f32", "f16", "bf16"]
INT_OF = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}
E8M0 = getattr(torch, "float8_e8m0fnu", torch.uint8)
FP4X2 = getattr(torch, "float4_e2m1fn_x2", torch.uint8)
EPS = 1e-6

make = MX.make


def up4(n):
    return (n + 3) // 4 * 4


def ocols(cols, fmt):
    return cols // 2 if fmt == "mxfp4" else cols


def u8(t):
    return t.view(torch.uint8).cpu().numpy()


def check_exact(q, s, want_s, want_q, what="", loose=None):
    """device element bytes and scale bytes against the reference, byte for byte; loose (MXFP8 only): the elements whose NaN came from two
    NaNs - compared without the sign bit"""
    g, gs = u8(q).reshape(want_q.shape), u8(s).reshape(want_s.shape)
    bad = np.argwhere(gs != want_s)
    assert bad.shape[0] == 0, (what, "scales", bad.shape[0], [(int(r), int(c), int(gs[r, c]), int(want_s[r, c])) for r, c in bad[:6]])
    if loose is not None:
        g, want_q = np.where(loose, g & 0x7F, g), np.where(loose, want_q & 0x7F, want_q)
    bad = np.argwhere(g != want_q)
    assert bad.shape[0] == 0, (what, bad.shape[0], [(int(r), int(c), hex(int(g[r, c])), hex(int(want_q[r, c]))) for r, c in bad[:6]])


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(INT_OF[a.dtype]), b.contiguous().view(INT_OF[b.dtype]))


def check_op_outputs(q, s, rows, cols, fmt):
    """the op layer's types, shapes and the padded scale allocation with its 2^0 pad bytes"""
    nb = cols // 32
    assert q.shape == (rows, ocols(cols, fmt)) and q.dtype == (FP4X2 if fmt == "mxfp4" else torch.uint8) and q.is_contiguous()
    assert s.shape == (rows, nb) and s.dtype == E8M0
    if rows > 1:
        assert s.stride() == (up4(nb), 1)
    if nb % 4:
        whole = torch.as_strided(s.view(torch.uint8), (rows, up4(nb)), (up4(nb), 1))
        assert whole[:, nb:].eq(0x7F).all(), "pad scale bytes are 2^0"


def act_raw(x_ptr, dt, rows, cols, ld_in, act, out_ptr, ld_out, s_ptr, ld_s, fmt):
    rc = L.load().fp8mi_act_quantize_mx(x_ptr, CODE[dt], rows, cols, ld_in, act, out_ptr, ld_out, s_ptr, ld_s, FMT[fmt], torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.load().fp8mi_last_error()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# 1. act="none": the full grid, no tolerance
# ---------------------------------------------------------------------------------------------------------------------------

COLS = [32, 64, 96, 128, 160, 224, 1024, 4096, 4128, 8224, 16384, 16416]
ROWS = [1, 3, 5, 257]


@pytest.mark.parametrize("fmt", MX.FORMATS)
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("gated", [False, True], ids=["ungated", "gated"])
def test_none_grid_is_exact(native, cuda, gated, dt, fmt):
    """One wave per row, several waves per row, eight waves for fp32 beyond 8192 columns, the looping form (16416); one, two, three blocks
    and rows whose block count is no multiple of four (pad scale bytes).  Ungated: also the stand-alone quantiser, on the device."""
    rng = np.random.default_rng(1000 * gated + 100 * CODE[dt] + FMT[fmt])
    for cols in COLS:
        for rows in ROWS:
            x = make(rng, rows, 2 * cols if gated else cols, dt)
            xd = x.to(cuda)
            q, s = native.fp8_act_quantize(xd, "none", gated, fmt)
            check_op_outputs(q, s, rows, cols, fmt)
            ws, wq, _ = MX.act_mx_ref(x, "none", gated, fmt)
            check_exact(q, s, ws, wq, what=f"{fmt} {dt} gated={gated} {rows}x{cols}")
            if not gated:
                dq, ds = (native.fp8_quantize_mxfp8 if fmt == "mxfp8" else native.fp8_quantize_mxfp4)(xd)
                assert dq.dtype == q.dtype and ds.dtype == s.dtype
                assert torch.equal(q.view(torch.uint8), dq.view(torch.uint8)) and torch.equal(s.view(torch.uint8), ds.view(torch.uint8)), (rows, cols)


def test_shapes_and_leading_dimensions_of_the_op(native, cuda):
    rng = np.random.default_rng(7)
    x = make(rng, 12, 448, torch.bfloat16).reshape(3, 4, 448)
    for fmt in MX.FORMATS:
        q, s = native.fp8_act_quantize(x.to(cuda), "none", True, fmt)
        assert q.shape == (3, 4, ocols(224, fmt)) and s.shape == (3, 4, 7) and s.dtype == E8M0
        ws, wq, _ = MX.act_mx_ref(x.reshape(12, 448), "none", True, fmt)
        check_exact(q, s, ws, wq, f"3-D gated {fmt}")
        v = make(rng, 1, 96, torch.float32).reshape(96)
        q, s = native.fp8_act_quantize(v.to(cuda), scale=fmt)
        assert q.shape == (ocols(96, fmt),) and s.shape == (3,)
        ws, wq, _ = MX.act_mx_ref(v.reshape(1, 96), "none", False, fmt)
        check_exact(q, s, ws, wq, f"1-D {fmt}")
        with pytest.raises(AssertionError, match="multiple of 32"):
            native.fp8_act_quantize(torch.zeros(4, 48, device=cuda), scale=fmt)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the normalisations: every variant, exact against the reference fed with the returned statistics
# ---------------------------------------------------------------------------------------------------------------------------

N_COLS = [32, 224, 1024, 4128, 16416]
VARIANTS = ["plain", "weight", "weight_bias", "mod", "residual", "all"]


def variant_inputs(rng, variant, rows, cols, dt, pdt, rows_per_mod=2):
    kw = {}
    if variant in ("weight", "weight_bias", "all"):
        kw["weight"] = NR.make_params(rng, 1, cols, pdt, 1.0)[0]
    if variant in ("weight_bias", "all"):
        kw["bias"] = NR.make_params(rng, 1, cols, pdt)[0]
    if variant in ("mod", "all"):
        nmod = -(-rows // rows_per_mod)     # rows_per_mod does not divide 3, 5 or 257 rows
        kw["mod_scale"], kw["mod_shift"], kw["rows_per_mod"] = NR.make_params(rng, nmod, cols, pdt), NR.make_params(rng, nmod, cols, pdt), rows_per_mod
    if variant in ("residual", "all"):
        kw["residual"] = NR.make_rows(rng, rows, cols, dt)
    return kw


def ptr(t):
    return None if t is None else t.data_ptr()


def norm_raw(cuda, x, norm, fmt, ld_s=None, eps=EPS, weight=None, bias=None, mod_scale=None, mod_shift=None, rows_per_mod=1, residual=None):
    """The C entry point on contiguous device copies of CPU tensors -> dict of device results (q, s as (rows, ld_s) bytes, mean, rstd, h)"""
    rows, cols = x.shape
    dev = lambda t: None if t is None else t.to(cuda).contiguous()   # noqa: E731
    xd, w, b, msc, msh, res = dev(x), dev(weight), dev(bias), dev(mod_scale), dev(mod_shift), dev(residual)
    params = [t for t in (w, b, msc, msh) if t is not None]
    pdt = params[0].dtype if params else x.dtype
    nb = cols // 32
    ld_s = nb if ld_s is None else ld_s
    q = torch.empty((rows, ocols(cols, fmt)), dtype=torch.uint8, device=cuda)
    s = torch.full((rows, ld_s), 0xEE, dtype=torch.uint8, device=cuda)
    layer = norm == "layer"
    mean = torch.full((rows,), 7.0, dtype=torch.float32, device=cuda) if layer else None
    rstd = torch.full((rows,), 7.0, dtype=torch.float32, device=cuda)
    h = None if res is None else torch.empty_like(res)
    ld = max(cols, 1)
    rc = L.load().fp8mi_norm_quantize_mx(xd.data_ptr(), CODE[x.dtype], rows, cols, ld, NORM[norm], eps, ptr(w), ptr(b), ptr(msc), ptr(msh), ld, rows_per_mod,
                                         CODE[pdt], ptr(res), ld, ptr(h), ld, q.data_ptr(), max(q.shape[1], 1), s.data_ptr(), max(ld_s, 1), FMT[fmt],
                                         ptr(mean), rstd.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.load().fp8mi_last_error()
    torch.cuda.synchronize()
    return dict(q=q, s=s, mean=mean, rstd=rstd, h=h)


def norm_verify(got, x, norm, fmt, what, eps=EPS, masked=False, **kw):
    """statistics within their caps (as tests/test_gpu_norm_quant.py holds them); then element bytes, scale bytes, pad bytes and h exact
    against the reference fed with the returned statistics"""
    rows, cols = x.shape
    nb = cols // 32
    h_ref, stored = NR.norm_h(x, kw.get("residual"))
    mean = None if got["mean"] is None else got["mean"].cpu().numpy()
    rstd = got["rstd"].cpu().numpy()
    mr, rr = NR.stat_ratios(h_ref, norm, eps, mean, rstd)
    assert mr <= 1.0 and rr <= 1.0, (what, "statistics", mr, rr)
    ws, wq, y, _ = MX.norm_mx_ref(x, norm, fmt, mean=mean, rstd=rstd, eps=eps, **kw)
    loose = NR.two_nan_elements(x, norm, kw.get("residual"), mean, rstd) if masked and fmt == "mxfp8" else None
    s = got["s"]
    check_exact(got["q"], s[:, :nb].contiguous(), ws, wq, what, loose=loose)
    if s.shape[1] > nb:      # the scale row is wider than the blocks: 2^0 up to the next multiple of four if that fits, untouched beyond
        pad = up4(nb) if s.shape[1] >= up4(nb) else nb
        assert s[:, nb:pad].eq(0x7F).all() and s[:, pad:].eq(0xEE).all(), (what, "scale bytes past the blocks")
    if stored is not None:
        assert same(got["h"].cpu(), stored), (what, "h_out")
    return mr, rr


def run_norm_grid(cuda, dt, norm, fmt, variant_of, pdt_of, seed):
    worst = [0.0, 0.0]
    for ci, cols in enumerate(N_COLS):
        for ri, rows in enumerate(ROWS):
            rng = np.random.default_rng(seed + 7 * cols + rows)
            x = NR.make_rows(rng, rows, cols, dt, norm == "layer")
            variant, pdt = variant_of(ci, ri), pdt_of(ci, ri)
            kw = variant_inputs(rng, variant, rows, cols, dt, pdt)
            nb = cols // 32
            ld_s = (nb, up4(nb), up4(nb) + 3)[(ci + ri) % 3]       # exactly the blocks; torch's padded row; wider and odd (byte stores)
            got = norm_raw(cuda, x, norm, fmt, ld_s=ld_s, **kw)
            mr, rr = norm_verify(got, x, norm, fmt, f"{norm} {dt} {variant} params {pdt} {fmt} {rows}x{cols} ld_s {ld_s}", **kw)
            worst = [max(worst[0], mr), max(worst[1], rr)]
    print(f"[mx_fused norm] {norm} {dt} {fmt}: mean at {worst[0]:.3f} of its cap, rstd at {worst[1]:.3f}")


@pytest.mark.parametrize("fmt", MX.FORMATS)
@pytest.mark.parametrize("norm", ["rms", "layer"])
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_norm_grid_variants_spread(cuda, dt, norm, fmt):
    """Register-resident with one wave per row and with several, eight for fp32 (16416 loops in every dtype); the six variants rotate over
    columns and rows, shifted by dtype, norm and format; the parameters of 16-bit input are fp32 in every other cell."""
    off = CODE[dt] + 2 * FMT[fmt] + NORM[norm]
    run_norm_grid(cuda, dt, norm, fmt, lambda ci, ri: VARIANTS[(ci + ri + off) % 6], lambda ci, ri: torch.float32 if (ci + ri + off) % 2 else dt,
                  100000 * NORM[norm] + 10000 * CODE[dt] + 1000 * FMT[fmt])


@pytest.mark.parametrize("fmt", MX.FORMATS)
@pytest.mark.parametrize("norm", ["rms", "layer"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_norm_grid_bf16_every_variant(cuda, variant, norm, fmt):
    run_norm_grid(cuda, torch.bfloat16, norm, fmt, lambda ci, ri: variant, lambda ci, ri: torch.bfloat16 if (ci + ri) % 3 else torch.float32,
                  500000 + 100000 * NORM[norm] + 1000 * FMT[fmt] + 17 * VARIANTS.index(variant))


def test_norm_op_returns_scales_h_and_stats(native, cuda):
    rng = np.random.default_rng(61)
    B, T, C = 2, 5, 224
    x = NR.make_rows(rng, B * T, C, torch.bfloat16, True).reshape(B, T, C)
    res = NR.make_rows(rng, B * T, C, torch.bfloat16).reshape(B, T, C)
    w, b = NR.make_params(rng, 1, C, torch.bfloat16, 1.0)[0], NR.make_params(rng, 1, C, torch.bfloat16)[0]
    msc, msh = NR.make_params(rng, B, C, torch.bfloat16), NR.make_params(rng, B, C, torch.bfloat16)
    for fmt in MX.FORMATS:
        q, s, h, rstd, mean = native.fp8_norm_quantize(x.to(cuda), "layer", w.to(cuda), b.to(cuda), EPS, res.to(cuda), msc.to(cuda), msh.to(cuda), fmt,
                                                       return_stats=True)
        assert q.shape == (B, T, ocols(C, fmt)) and s.shape == (B, T, 7) and s.dtype == E8M0 and h.shape == (B, T, C) and rstd.shape == (B, T, 1)
        ws, wq, _, stored = MX.norm_mx_ref(x.reshape(-1, C), "layer", fmt, mean=mean.cpu().numpy(), rstd=rstd.cpu().numpy(), eps=EPS, weight=w, bias=b,
                                           residual=res.reshape(-1, C), mod_scale=msc, mod_shift=msh, rows_per_mod=T)
        check_exact(q, s, ws, wq, f"op {fmt}")
        assert same(h.reshape(-1, C).cpu(), stored)
        q2, s2 = native.fp8_norm_quantize(x.to(cuda), "rms", scale=fmt)
        assert q2.shape == q.shape and s2.shape == s.shape


# ---------------------------------------------------------------------------------------------------------------------------
# 3. layout edges through the C entry points
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", MX.FORMATS)
@pytest.mark.parametrize("gated", [False, True], ids=["ungated", "gated"])
def test_leading_dimensions_and_untouched_padding(cuda, gated, fmt):
    """ld_in, ld_out and ld_s larger than needed - aligned (vector forms, dword scale stores) and odd (any-alignment form, byte stores) -
    the input inside a NaN-filled buffer, the outputs inside 0xA5- / 0xEE-filled ones.  The pad scale bytes are 0x7F when ld_s has room
    for round_up(cols / 32, 4); with ld_s == cols / 32 (no multiple of four) exactly cols / 32 bytes per row are written."""
    rng = np.random.default_rng(11 + 2 * gated + FMT[fmt])
    act = L.ACT_NONE | (L.ACT_GATED if gated else 0)
    dts = {0: torch.bfloat16, 1: torch.float32, 2: torch.float16}
    # (rows, cols, extra ld_in, extra ld_out, ld_s - cols / 32)
    cases = ((37, 992, 24, 8, 1), (37, 992, 1, 3, 0), (5, 3104, 1024, 0, 3), (5, 3104, 0, 8, 2), (3, 20000, 480, 16, 7), (2, 20000, 1, 0, 0),
             (9, 32, 0, 1, 0), (4, 12320, 8, 16, 3), (6, 224, 56, 0, 1), (7, 96, 0, 0, 0), (1, 160, 3, 5, 0), (6, 4128, 16, 8, 4))
    for i, (rows, cols, pad_in, pad_out, pad_s) in enumerate(cases):
        dt = dts[i % 3]
        width, oc, nb = (2 * cols if gated else cols), ocols(cols, fmt), cols // 32
        ld_in, ld_out, ld_s = width + pad_in, oc + pad_out, nb + pad_s
        x = make(rng, rows, width, dt)
        buf = torch.full((rows, ld_in), float("nan"), dtype=dt, device=cuda)
        buf[:, :width] = x.to(cuda)
        out = torch.full((rows * ld_out + 64,), 0xA5, dtype=torch.uint8, device=cuda)
        sc = torch.full((rows * ld_s + 16,), 0xEE, dtype=torch.uint8, device=cuda)
        act_raw(buf.data_ptr(), dt, rows, cols, ld_in, act, out.data_ptr(), ld_out, sc.data_ptr(), ld_s, fmt)
        what = f"{fmt} {rows}x{cols} {dt} ld_in {ld_in} ld_out {ld_out} ld_s {ld_s}"
        o2, s2 = out[:rows * ld_out].reshape(rows, ld_out), sc[:rows * ld_s].reshape(rows, ld_s)
        ws, wq, _ = MX.act_mx_ref(x, "none", gated, fmt)
        check_exact(o2[:, :oc].contiguous(), s2[:, :nb].contiguous(), ws, wq, what)
        assert o2[:, oc:].eq(0xA5).all() and out[rows * ld_out:].eq(0xA5).all(), (what, "padding bytes written")
        pad = up4(nb) if ld_s >= up4(nb) else nb
        assert s2[:, nb:pad].eq(0x7F).all(), (what, "pad scale bytes are 2^0")
        assert s2[:, pad:].eq(0xEE).all() and sc[rows * ld_s:].eq(0xEE).all(), (what, "scale bytes written past the row")


@pytest.mark.parametrize("fmt", MX.FORMATS)
@pytest.mark.parametrize("gated", [False, True], ids=["ungated", "gated"])
def test_pointers_offset_by_one_and_two_elements(cuda, gated, fmt):
    """Input, output and scale pointers off their alignment take the any-alignment form and byte scale stores; the bytes around stay."""
    rng = np.random.default_rng(21 + 2 * gated + FMT[fmt])
    act = L.ACT_NONE | (L.ACT_GATED if gated else 0)
    for dt in (torch.bfloat16, torch.float32):
        esz = torch.empty(0, dtype=dt).element_size()
        for rows, cols in ((1, 4992), (6, 1024), (3, 17024), (5, 32)):
            width, oc, nb = (2 * cols if gated else cols), ocols(cols, fmt), cols // 32
            for off_in, off_out, off_s in ((1, 0, 0), (0, 1, 0), (1, 1, 1), (2, 2, 2), (2, 0, 0), (0, 0, 1)):
                x = make(rng, rows, width, dt)
                buf = torch.zeros(rows * width + 8, dtype=dt, device=cuda)
                buf[off_in:off_in + rows * width].copy_(x.reshape(-1).to(cuda))
                out = torch.full((rows * oc + 16,), 0x5A, dtype=torch.uint8, device=cuda)
                sc = torch.full((rows * nb + 16,), 0xEE, dtype=torch.uint8, device=cuda)
                act_raw(buf.data_ptr() + off_in * esz, dt, rows, cols, width, act, out.data_ptr() + off_out, oc, sc.data_ptr() + off_s, nb, fmt)
                ws, wq, _ = MX.act_mx_ref(x, "none", gated, fmt)
                check_exact(out[off_out:off_out + rows * oc].contiguous(), sc[off_s:off_s + rows * nb].contiguous(), ws, wq,
                            what=f"{fmt} {dt} {rows}x{cols} offsets {off_in} {off_out} {off_s}")
                assert out[:off_out].eq(0x5A).all() and out[off_out + rows * oc:].eq(0x5A).all()
                # ld_s == cols / 32: nothing past the blocks (a row of these shapes that is a multiple of four blocks has no pad bytes either)
                assert sc[:off_s].eq(0xEE).all() and sc[off_s + rows * nb:].eq(0xEE).all()


def test_norm_leading_dimensions_and_offsets(cuda):
    """fp8mi_norm_quantize_mx with every leading dimension larger than the row and with x one element off its alignment."""
    rng = np.random.default_rng(31)
    nan = float("nan")
    for i, (rows, cols, pads, rpm) in enumerate(((37, 992, (24, 8, 16, 40, 8, 1), 3), (5, 3104, (1, 3, 5, 7, 3, 0), 2), (3, 20000, (480, 16, 32, 8, 16, 7), 1),
                                                 (4, 4128, (8, 8, 8, 8, 4, 3), 3), (7, 96, (0, 0, 0, 0, 0, 0), 7))):
        for fmt in MX.FORMATS:
            for norm in ("rms", "layer"):
                dt = (torch.bfloat16, torch.float32, torch.float16)[i % 3]
                pdt = dt if i % 2 else torch.float32
                p_in, p_res, p_h, p_mod, p_out, p_s = pads
                x = NR.make_rows(rng, rows, cols, dt, norm == "layer")
                kw = variant_inputs(rng, "all", rows, cols, dt, pdt, rows_per_mod=rpm)
                oc, nb = ocols(cols, fmt), cols // 32

                def padded(t, ld, fill):
                    b = torch.full((t.shape[0], ld), fill, dtype=t.dtype, device=cuda)
                    b[:, :t.shape[1]] = t.to(cuda)
                    return b
                xb, rb = padded(x, cols + p_in, nan), padded(kw["residual"], cols + p_res, nan)
                mscb, mshb = padded(kw["mod_scale"], cols + p_mod, nan), padded(kw["mod_shift"], cols + p_mod, nan)
                w, b = kw["weight"].to(cuda), kw["bias"].to(cuda)
                ld_out, ld_h, ld_s = oc + p_out, cols + p_h, nb + p_s
                out = torch.full((rows * ld_out + 64,), 0xA5, dtype=torch.uint8, device=cuda)
                sc = torch.full((rows, ld_s), 0xEE, dtype=torch.uint8, device=cuda)
                hb = torch.full((rows, ld_h), nan, dtype=dt, device=cuda)
                mean = torch.empty(rows, dtype=torch.float32, device=cuda) if norm == "layer" else None
                rstd = torch.empty(rows, dtype=torch.float32, device=cuda)
                rc = L.load().fp8mi_norm_quantize_mx(xb.data_ptr(), CODE[dt], rows, cols, cols + p_in, NORM[norm], EPS, w.data_ptr(), b.data_ptr(),
                                                     mscb.data_ptr(), mshb.data_ptr(), cols + p_mod, rpm, CODE[pdt], rb.data_ptr(), cols + p_res, hb.data_ptr(),
                                                     ld_h, out.data_ptr(), ld_out, sc.data_ptr(), ld_s, FMT[fmt], ptr(mean), rstd.data_ptr(),
                                                     torch.cuda.current_stream().cuda_stream)
                assert rc == 0, L.load().fp8mi_last_error()
                torch.cuda.synchronize()
                what = f"{fmt} {norm} {rows}x{cols} {dt} pads {pads}"
                o2 = out[:rows * ld_out].reshape(rows, ld_out)
                got = dict(q=o2[:, :oc].contiguous(), s=sc, mean=mean, rstd=rstd, h=hb[:, :cols].contiguous())
                norm_verify(got, x, norm, fmt, what, **kw)
                assert o2[:, oc:].eq(0xA5).all() and out[rows * ld_out:].eq(0xA5).all(), (what, "padding bytes written")
                assert torch.isnan(hb[:, cols:]).all(), (what, "h_out padding written")
    # x one and two elements off its alignment: the any-alignment form
    for fmt in MX.FORMATS:
        for dt, rows, cols, off in ((torch.bfloat16, 6, 1024, 1), (torch.float32, 3, 17024, 1), (torch.float16, 5, 224, 2)):
            x = NR.make_rows(rng, rows, cols, dt, True)
            buf = torch.zeros(rows * cols + 8, dtype=dt, device=cuda)
            buf[off:off + rows * cols].copy_(x.reshape(-1).to(cuda))
            oc, nb = ocols(cols, fmt), cols // 32
            q = torch.empty((rows, oc), dtype=torch.uint8, device=cuda)
            sc = torch.full((rows, nb), 0xEE, dtype=torch.uint8, device=cuda)
            mean, rstd = torch.empty(rows, dtype=torch.float32, device=cuda), torch.empty(rows, dtype=torch.float32, device=cuda)
            rc = L.load().fp8mi_norm_quantize_mx(buf.data_ptr() + off * buf.element_size(), CODE[dt], rows, cols, cols, L.NORM_LAYER, EPS, None, None, None, None,
                                                 cols, 1, CODE[dt], None, cols, None, cols, q.data_ptr(), oc, sc.data_ptr(), nb, FMT[fmt], mean.data_ptr(),
                                                 rstd.data_ptr(), torch.cuda.current_stream().cuda_stream)
            assert rc == 0, L.load().fp8mi_last_error()
            torch.cuda.synchronize()
            norm_verify(dict(q=q, s=sc, mean=mean, rstd=rstd, h=None), x, "layer", fmt, f"{fmt} {dt} {rows}x{cols} offset {off}")


def test_column_slice_view_through_the_python_op(native, cuda):
    rng = np.random.default_rng(33)
    wide = make(rng, 40, 4096, torch.bfloat16)
    wd = wide.to(cuda)
    for c0, width in ((512, 3072), (8, 1024), (3, 192), (1, 4032), (0, 4096)):
        for gated in (False, True):
            for fmt in MX.FORMATS:
                q, s = native.fp8_act_quantize(wd[:, c0:c0 + width], "none", gated, fmt)
                check_op_outputs(q, s, 40, width // 2 if gated else width, fmt)
                ws, wq, _ = MX.act_mx_ref(wide[:, c0:c0 + width], "none", gated, fmt)
                check_exact(q, s, ws, wq, what=f"slice {c0}+{width} {gated} {fmt}")
        for fmt in MX.FORMATS:
            q, s, rstd = native.fp8_norm_quantize(wd[:, c0:c0 + width], "rms", scale=fmt, return_stats=True)
            ws, wq, _, _ = MX.norm_mx_ref(wide[:, c0:c0 + width], "rms", fmt, rstd=rstd.cpu().numpy(), eps=EPS)
            check_exact(q, s, ws, wq, what=f"norm slice {c0}+{width} {fmt}")


# ---------------------------------------------------------------------------------------------------------------------------
# 4. non-finite input
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", MX.FORMATS)
def test_zero_nan_inf_and_tiny_blocks_follow_the_recipe(native, cuda, fmt):
    rng = np.random.default_rng(41 + FMT[fmt])
    nan_code = 0x7F if fmt == "mxfp8" else 0xC
    for dt, cols, gated in ((torch.float32, 800, False), (torch.bfloat16, 3104, True), (torch.float16, 12320, True), (torch.bfloat16, 20000, False),
                            (torch.float32, 64, True), (torch.bfloat16, 224, True), (torch.float32, 16416, True)):
        width, last = (2 * cols if gated else cols), cols - 1
        x = make(rng, 14, width, dt)
        x[1] = 0.0                                    # all-zero rows and blocks: scale byte 0, bytes 0
        x[7, :32] = 0.0
        x[7, 5] = -0.0
        x[3, 5] = float("nan")                        # a NaN: scale 0xFF for its block only
        x[3, last] = -float("nan")
        x[4, :cols] = float("nan")
        x[5, 0], x[5, 1] = float("nan"), 3.0e4
        x[8, 9] = float("inf")                        # an inf: the largest scale, the element saturates
        x[9, last] = float("-inf")
        x[10, 3], x[10, 4] = float("inf"), float("nan")
        if dt != torch.float16:                       # a block of values below 1e-36 (fp32 subnormal descale)
            x[6, 32:64] = torch.from_numpy((rng.standard_normal(32) * 1e-37).astype(np.float32)).to(dt)
            x[6, 33] = 1.0e-40
        if gated:
            x[2, cols + 6] = float("nan")
            x[11, 8], x[11, cols + 8] = 0.0, float("inf")           # 0 * inf is a NaN element
            x[12, cols + 40 % cols], x[12, 40 % cols] = 0.0, float("-inf")
            x[13, cols:] = 0.0
        q, s = native.fp8_act_quantize(x.to(cuda), "none", gated, fmt)
        ws, wq, _ = MX.act_mx_ref(x, "none", gated, fmt)
        check_exact(q, s, ws, wq, what=f"specials {fmt} {dt} {cols} gated {gated}")
        g, gs = u8(q), u8(s)
        el = (lambda r, c: int(g[r, c]) & 0x7F) if fmt == "mxfp8" else (lambda r, c: (int(g[r, c // 2]) >> (4 * (c & 1))) & 0xF)
        assert (gs[1] == 0).all() and (g[1] == 0).all() and gs[7, 0] == 0
        assert gs[3, 0] == 0xFF and gs[3, -1] == 0xFF and el(3, 5) == nan_code and el(3, last) == nan_code
        if cols > 64:
            assert (gs[3, 1:-1] != 0xFF).all()
        assert (gs[4] == 0xFF).all() and gs[8, 0] == 254 and gs[9, -1] == 254 and gs[10, 0] == 0xFF
        if gated:
            assert gs[11, 0] == 0xFF and el(11, 8) == nan_code and (gs[13] == 0).all()


@pytest.mark.parametrize("fmt", MX.FORMATS)
@pytest.mark.parametrize("norm", ["rms", "layer"])
def test_norm_special_rows(cuda, norm, fmt):
    """A NaN or (LayerNorm) an inf makes the whole row NaN - every scale byte 0xFF; RMSNorm with an inf: rstd 0, zeros and NaNs; an
    all-zero row.  The sign bit of a NaN byte that two NaNs generated is set aside (MXFP8; the MXFP4 code of a NaN has one form)."""
    rng = np.random.default_rng(51 + NORM[norm] + FMT[fmt])
    for dt, cols in ((torch.bfloat16, 1024), (torch.float32, 224), (torch.float16, 4128), (torch.float32, 16416)):
        x = NR.make_rows(rng, 6, cols, dt, norm == "layer")
        x[1, 7] = float("nan")
        x[2, cols - 1] = float("inf")
        x[3] = 0.0
        x[4, 0], x[4, 40] = float("-inf"), float("nan")
        kw = variant_inputs(rng, "weight", 6, cols, dt, torch.float32)
        got = norm_raw(cuda, x, norm, fmt, ld_s=up4(cols // 32), **kw)
        norm_verify(got, x, norm, fmt, f"specials {norm} {fmt} {dt} {cols}", masked=True, **kw)
        gs = u8(got["s"])[:, :cols // 32]
        assert (gs[1] == 0xFF).all() and (gs[4] == 0xFF).all() and (gs[0] != 0xFF).all()
        if norm == "layer":
            assert (gs[2] == 0xFF).all()
        else:
            assert gs[2, -1] == 0xFF and (gs[2, :-1] == 0).all()      # rstd = 0: zeros, and inf * 0 in the last block


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the transcendental activations against the float64 reference
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("gated", [False, True], ids=["ungated", "gated"])
@pytest.mark.parametrize("act", MX.T_ACTS)
def test_transcendental_acts_against_float64(native, cuda, act, gated, dt):
    """Both formats on every form.  The caps are conditions, not measurements; what the GPU gives is printed."""
    worst = {f: [0.0, 0.0, 0] for f in MX.FORMATS}
    for rows, cols, x in MX.t_inputs(act, gated, dt):
        xd = x.to(cuda)
        y = MX.A.act_y(x, act, gated)
        for fmt in MX.FORMATS:
            q, s = native.fp8_act_quantize(xd, act, gated, fmt)
            r = MX.compare_transcendental(y, u8(s), u8(q), fmt)
            took = int((u8(s).reshape(rows, -1) != MX.to_mx_ref(y, fmt)[0]).sum())
            share, excused = r["off_by_one"] / r["elements"], r["excused"] / r["blocks"]
            worst[fmt] = [max(worst[fmt][0], share), max(worst[fmt][1], excused), worst[fmt][2] + took]
            print(f"[mx_fused] {act} gated={gated} {dt} {fmt} {rows}x{cols}: codes one step off {share:.2e}, blocks inside the window {r['excused']} of "
                  f"{r['blocks']} ({excused:.2%}), of which {took} took the neighbouring exponent")
            what = (act, gated, dt, fmt, rows, cols, r)
            assert r["wrong_scale"] == 0, what
            assert r["far"] == 0 and r["off_by_one"] <= MX.BYTE_SHARE * r["elements"], what
            assert r["excused"] <= max(1, MX.BLOCK_SHARE * r["blocks"]), what
    for fmt, (share, excused, took) in worst.items():
        print(f"[mx_fused numerics] {act:9s} gated={int(gated)} {str(dt)[6:]:8s} {fmt}: largest share of codes one step off {share:.2e}, largest share of "
              f"blocks inside the window {excused:.2%}, blocks that took the neighbouring exponent {took}")


# ---------------------------------------------------------------------------------------------------------------------------
# 6. rows are independent, calls repeat
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", MX.FORMATS)
def test_rows_are_independent_and_calls_repeat(native, cuda, fmt):
    rng = np.random.default_rng(4500 + FMT[fmt])
    for dt, rows, cols, gated, act in ((torch.bfloat16, 257, 1024, True, "silu"), (torch.float16, 37, 4128, True, "gelu_tanh"),
                                       (torch.float32, 21, 16384, False, "gelu_erf"), (torch.bfloat16, 9, 16416, True, "silu"),
                                       (torch.float32, 33, 160, True, "gelu_tanh"), (torch.bfloat16, 64, 96, False, "gelu_erf")):
        x = make(rng, rows, 2 * cols if gated else cols, dt).to(cuda)
        perm = torch.from_numpy(rng.permutation(rows)).to(cuda)
        q, s = native.fp8_act_quantize(x, act, gated, fmt)
        q2, s2 = native.fp8_act_quantize(x, act, gated, fmt)
        assert torch.equal(q.view(torch.uint8), q2.view(torch.uint8)) and torch.equal(s.view(torch.uint8), s2.view(torch.uint8)), (dt, rows, cols, "repeat")
        qp, sp = native.fp8_act_quantize(x[perm].contiguous(), act, gated, fmt)
        assert torch.equal(qp.view(torch.uint8), q.view(torch.uint8)[perm]) and torch.equal(sp.view(torch.uint8), s.view(torch.uint8)[perm]), (dt, rows, cols, "perm")
        if not gated:
            w = NR.make_params(rng, 1, cols, dt, 1.0)[0].to(cuda)
            n1, n2 = native.fp8_norm_quantize(x, "layer", w, scale=fmt), native.fp8_norm_quantize(x, "layer", w, scale=fmt)
            npm = native.fp8_norm_quantize(x[perm].contiguous(), "layer", w, scale=fmt)
            for a, b, c in zip(n1, n2, npm):
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)) and torch.equal(c.view(torch.uint8), a.view(torch.uint8)[perm]), (dt, rows, cols, "norm")


# ---------------------------------------------------------------------------------------------------------------------------
# 7. graph capture, empty shapes
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", MX.FORMATS)
@pytest.mark.parametrize("rows,cols", [(128, 3072), (16, 14336), (4, 20000)], ids=["wave-per-row", "workgroup-per-row", "looping"])
def test_launches_replay_in_a_graph(native, cuda, rows, cols, fmt):
    """Captured once, replayed twice on new data, byte for byte; an eager call of each op is ONE launch."""
    rng = np.random.default_rng(rows + cols + FMT[fmt])
    xs = make(rng, rows, 2 * cols, torch.bfloat16).to(cuda)
    xn = xs[:, :cols].contiguous()
    w = NR.make_params(rng, 1, cols, torch.bfloat16, 1.0)[0]
    wd = w.to(cuda)
    with L.kernel_timer(8) as prof:
        native.fp8_act_quantize(xs, "none", True, fmt)
    torch.cuda.synchronize()
    assert len(prof.ms) == 1, "one launch"
    with L.kernel_timer(8) as prof:
        native.fp8_norm_quantize(xn, "rms", wd, scale=fmt, return_stats=True)
    torch.cuda.synchronize()
    assert len(prof.ms) == 1, "one launch"
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        q, s = native.fp8_act_quantize(xs, "none", True, fmt)
        nq, ns, rstd = native.fp8_norm_quantize(xn, "rms", wd, scale=fmt, return_stats=True)
    for _ in range(2):
        x = make(rng, rows, 2 * cols, torch.bfloat16)
        xs.copy_(x.to(cuda))
        xn.copy_(x[:, :cols].to(cuda))
        g.replay()
        torch.cuda.synchronize()
        ws, wq, _ = MX.act_mx_ref(x, "none", True, fmt)
        check_exact(q, s, ws, wq, what=f"graph replay {fmt} {rows}x{cols}")
        ws, wq, _, _ = MX.norm_mx_ref(x[:, :cols], "rms", fmt, rstd=rstd.cpu().numpy(), eps=EPS, weight=w)
        check_exact(nq, ns, ws, wq, what=f"graph replay norm {fmt} {rows}x{cols}")


def test_empty_shapes(native, cuda):
    lib = L.load()
    stream = torch.cuda.current_stream().cuda_stream
    for fmt in MX.FORMATS:
        assert lib.fp8mi_act_quantize_mx(None, L.BF16, 0, 128, 256, L.ACT_SILU | L.ACT_GATED, None, 128, None, 4, FMT[fmt], stream) == 0
        assert lib.fp8mi_act_quantize_mx(None, L.BF16, 5, 0, 0, L.ACT_SILU, None, 0, None, 0, FMT[fmt], stream) == 0
        assert lib.fp8mi_norm_quantize_mx(None, L.BF16, 0, 128, 128, L.NORM_RMS, EPS, None, None, None, None, 128, 1, L.BF16, None, 128, None, 128, None, 128, None,
                                          4, FMT[fmt], None, None, stream) == 0
        rstd = torch.full((6,), 7.0, dtype=torch.float32, device=cuda)
        assert lib.fp8mi_norm_quantize_mx(None, L.F32, 5, 0, 0, L.NORM_RMS, EPS, None, None, None, None, 0, 1, L.F32, None, 0, None, 0, None, 0, None, 0, FMT[fmt],
                                          None, rstd.data_ptr(), stream) == 0
        torch.cuda.synchronize()
        assert rstd.eq(7.0).all()            # nothing is written for cols == 0
        for gated in (False, True):
            q, s = native.fp8_act_quantize(torch.zeros(0, 64, dtype=torch.bfloat16, device=cuda), "silu", gated, fmt)
            assert q.shape == (0, ocols(32 if gated else 64, fmt)) and s.shape == (0, 1 if gated else 2)
        q, s = native.fp8_act_quantize(torch.zeros(4, 0, device=cuda), scale=fmt)
        assert q.shape == (4, 0) and s.shape == (4, 0)
        q, s = native.fp8_norm_quantize(torch.zeros(0, 64, dtype=torch.bfloat16, device=cuda), scale=fmt)
        assert q.shape == (0, ocols(64, fmt)) and s.shape == (0, 2)


# ---------------------------------------------------------------------------------------------------------------------------
# 8. the MLPs and norm-linears are their public steps, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------

MLP_SHAPES = [((70, 256, 384, 224), torch.bfloat16), ((1, 512, 128, 64), torch.float16), ((37, 416, 160, 288), torch.float32)]


def rel_fro(got, want):
    return float(np.linalg.norm(got.double().cpu().numpy() - want) / np.linalg.norm(want))


def recipe(native, fmt):
    """-> (weight quantiser, GEMM, linear, mlp, norm_linear, dequantiser) of a format"""
    if fmt == "mxfp8":
        return (native.fp8_quantize_mxfp8, native.fp8_scaled_mm_mxfp8, native.fp8_linear_mxfp8, native.fp8_mlp_mxfp8, native.fp8_norm_linear_mxfp8,
                native.fp8_dequantize_mxfp8)
    return (native.fp8_quantize_mxfp4, native.fp8_scaled_mm_mxfp4, native.fp8_linear_mxfp4, native.fp8_mlp_mxfp4, native.fp8_norm_linear_mxfp4,
            native.fp8_dequantize_mxfp4)


@pytest.mark.parametrize("gated", [False, True], ids=["ungated", "gated"])
@pytest.mark.parametrize("fmt", MX.FORMATS)
def test_mlps_are_their_public_steps(native, cuda, fmt, gated):
    quant, mm, linear, mlp, _, dequant = recipe(native, fmt)
    rng = np.random.default_rng(71 + gated + 2 * FMT[fmt])
    for (M, K, H, Nn), dt in MLP_SHAPES:
        x = make(rng, M, K, dt).to(cuda)
        w1 = torch.from_numpy((rng.standard_normal(((2 if gated else 1) * H, K)) / np.sqrt(K)).astype(np.float32)).to(cuda)
        w2 = torch.from_numpy((rng.standard_normal((Nn, H)) / np.sqrt(H)).astype(np.float32)).to(cuda)
        b1 = torch.from_numpy(rng.standard_normal(w1.shape[0]).astype(np.float32) * 0.1).to(cuda)
        b2 = torch.from_numpy(rng.standard_normal(Nn).astype(np.float32) * 0.1).to(cuda)
        (w1q, w1s), (w2q, w2s) = quant(w1), quant(w2)
        h = linear(x, w1q, w1s, b1)                       # the stand-alone quantiser of x: the same bytes as the fused launch with "none"
        assert h.dtype == dt and h.shape == (M, w1.shape[0])
        for act in ("none", "silu", "gelu_tanh"):
            got = mlp(x, w1q, w1s, w2q, w2s, act=act, gated=gated, bias1=b1, bias2=b2)
            assert got.shape == (M, Nn) and got.dtype == dt
            hq, hs = native.fp8_act_quantize(h, act, gated, fmt)
            assert same(got, mm(hq, w2q, hs, w2s, bias=b2, out_dtype=dt)), (fmt, gated, M, K, H, Nn, act, "public steps")
        if gated:       # act="none": also the composition through torch, then the stand-alone quantiser
            hq, hs = quant(h[:, :H].float() * h[:, H:].float())
            assert same(mlp(x, w1q, w1s, w2q, w2s, act="none", gated=True, bias1=b1, bias2=b2), mm(hq, w2q, hs, w2s, bias=b2, out_dtype=dt)), (fmt, M, "via torch")
        # silu against a float64 MLP on the dequantised weights: reported, not asserted
        got = mlp(x, w1q, w1s, w2q, w2s, act="silu", gated=gated, bias1=b1, bias2=b2)
        w1d, w2d = dequant(w1q, w1s).double().cpu(), dequant(w2q, w2s).double().cpu()
        h64 = x.double().cpu() @ w1d.t() + b1.double().cpu()
        a = MX.A.act64(h64[:, :H], "silu")
        want = ((a * h64[:, H:] if gated else a) @ w2d.t() + b2.double().cpu()).numpy()
        print(f"[mx_fused mlp] {fmt} gated={gated} {(M, K, H, Nn)} {dt}: rel. Frobenius distance to float64 {rel_fro(got, want):.4f}")
        assert torch.isfinite(got).all()
    # leading dimensions are kept
    K, H, Nn = 256, 384, 224
    x3 = make(rng, 6, K, torch.bfloat16).reshape(2, 3, K).to(cuda)
    w1 = torch.from_numpy((rng.standard_normal(((2 if gated else 1) * H, K)) / 16).astype(np.float32)).to(cuda)
    w2 = torch.from_numpy((rng.standard_normal((Nn, H)) / 20).astype(np.float32)).to(cuda)
    (w1q, w1s), (w2q, w2s) = quant(w1), quant(w2)
    y3 = mlp(x3, w1q, w1s, w2q, w2s, gated=gated)
    assert y3.shape == (2, 3, Nn) and y3.dtype == torch.bfloat16
    assert same(y3.reshape(6, Nn), mlp(x3.reshape(6, K), w1q, w1s, w2q, w2s, gated=gated))
    y32 = mlp(x3, w1q, w1s, w2q, w2s, act="gelu_erf", gated=gated, out_dtype=torch.float32)
    assert y32.shape == (2, 3, Nn) and y32.dtype == torch.float32 and torch.isfinite(y32).all()


@pytest.mark.parametrize("fmt", MX.FORMATS)
def test_norm_linears_are_their_public_steps(native, cuda, fmt):
    quant, mm, _, _, norm_linear, _ = recipe(native, fmt)
    rng = np.random.default_rng(81 + FMT[fmt])
    for (M, K, _, Nn), dt in MLP_SHAPES:
        B = 2 if M % 2 == 0 else 1
        x = NR.make_rows(rng, M, K, dt, True).reshape(B, M // B, K).to(cuda)
        res = NR.make_rows(rng, M, K, dt).reshape(B, M // B, K).to(cuda)
        w = torch.from_numpy((rng.standard_normal((Nn, K)) / np.sqrt(K)).astype(np.float32)).to(cuda)
        bias = torch.from_numpy(rng.standard_normal(Nn).astype(np.float32) * 0.1).to(cuda)
        nw, nb = NR.make_params(rng, 1, K, dt, 1.0)[0].to(cuda), NR.make_params(rng, 1, K, dt)[0].to(cuda)
        msc, msh = NR.make_params(rng, B, K, dt).to(cuda), NR.make_params(rng, B, K, dt).to(cuda)
        wq, ws = quant(w)
        for norm in ("rms", "layer"):
            y = norm_linear(x, wq, ws, norm, nw, bias=bias)
            q, s = native.fp8_norm_quantize(x, norm, nw, scale=fmt)
            assert y.shape == (B, M // B, Nn) and y.dtype == dt
            assert same(y.reshape(M, Nn), mm(q.reshape(M, -1), wq, s.reshape(M, -1), ws, bias=bias, out_dtype=dt)), (fmt, norm, M, K, Nn)
            y, h = norm_linear(x, wq, ws, norm, nw, nb, EPS, res, msc, msh, bias, torch.float32)
            q, s, h2 = native.fp8_norm_quantize(x, norm, nw, nb, EPS, res, msc, msh, fmt)
            assert y.dtype == torch.float32 and same(h, h2) and same(h, x + res)
            assert same(y.reshape(M, Nn), mm(q.reshape(M, -1), wq, s.reshape(M, -1), ws, bias=bias, out_dtype=torch.float32)), (fmt, norm, M, "all")


# ---------------------------------------------------------------------------------------------------------------------------
# 9. the patched torch._scaled_mm on the kernels' outputs
# ---------------------------------------------------------------------------------------------------------------------------

def test_scaled_mm_patch_on_the_kernels_outputs(cuda, patch, native):
    rng = np.random.default_rng(91)
    f8 = torch.float8_e4m3fn
    for M, H, Nn in ((256, 3072, 512), (64, 4096, 1024), (33, 1056, 160)):
        h = make(rng, M, 2 * H, torch.bfloat16).to(cuda)
        w = make(rng, Nn, H, torch.bfloat16).to(cuda)
        q, s = native.fp8_act_quantize(h, "silu", True, "mxfp8")
        wq, ws = native.fp8_quantize_mxfp8(w)
        got = torch._scaled_mm(q.view(f8), wq.view(f8).t(), scale_a=s, scale_b=ws, out_dtype=torch.bfloat16)
        want = native.fp8_scaled_mm_mxfp8(q, wq, s, ws, out_dtype=torch.bfloat16)
        torch.cuda.synchronize()
        assert got.dtype == torch.bfloat16 and torch.equal(got.view(torch.int16), want.view(torch.int16)), (M, H, Nn, "mxfp8")
        assert torch.isfinite(got).all()
        if FP4X2 is not torch.uint8:
            q, s = native.fp8_act_quantize(h, "silu", True, "mxfp4")
            wq, ws = native.fp8_quantize_mxfp4(w)
            got = torch._scaled_mm(q, wq.t(), scale_a=s, scale_b=ws, out_dtype=torch.bfloat16)
            want = native.fp8_scaled_mm_mxfp4(q, wq, s, ws, out_dtype=torch.bfloat16)
            torch.cuda.synchronize()
            assert torch.equal(got.view(torch.int16), want.view(torch.int16)) and torch.isfinite(got).all(), (M, H, Nn, "mxfp4")
