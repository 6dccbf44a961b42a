"""GPU: float8_e5m2 operands of the tensorwise / rowwise GEMM on every kernel family, the e5m2 casts, the _scaled_mm route and the C
ABI, against tests/e5m2_ref.py (torch CPU's decode / cast and a float64 matmul).

Tolerances (e5m2_ref.py): MM_TOL for the fp32-FMA kernels and for exact (narrow-range) cases on the matrix core; MFMA_TOL = 1e-3 x
sum|a||b| for random finite bytes on the matrix core - the truncation mechanism of profiles/mfma_numerics_r01.txt, which
profiles/mfma_numerics_e5m2.txt confirms for format code 1 (7 of 127 small products lost from 2^-14 below the largest of their group
of 8, for all four format pairs) - and MFMA_RMS_TOL = 1e-4 for rms(err) / rms(bound): measured 1.8e-5 .. 2.2e-5 at K = 128 and
falling with K on random finite bytes (same file), below half the gate, so the e4m3 gate is kept.  On top of the sum's bound the
checks allow the epilogue's own fp32 roundings (four, 2^-24 each, of |result| and |bias|) and one rounding to the output type."""
import os
import subprocess

import numpy as np
import pytest
import torch

import e5m2_ref as R
import fp8_mi355x_lib as L
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

E4, E5 = L.FMT_E4M3, L.FMT_E5M2
PAIRS = [(E5, E4), (E4, E5), (E5, E5)]
PAIR_IDS = ["e5m2xe4m3", "e4m3xe5m2", "e5m2xe5m2"]
TILE_KERNELS = [L.KERNEL_GEMM_128, L.KERNEL_GEMM_128x64, L.KERNEL_GEMM_256, L.KERNEL_GEMM_64x128, L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_32x64,
                L.KERNEL_GEMM_32x32, L.KERNEL_GEMM_128D]
WAVE_KERNELS = [L.KERNEL_GEMM_256W, L.KERNEL_GEMM_256x128W]
NAMES = {v: k for k, v in vars(L).items() if k.startswith("KERNEL_") and isinstance(v, int)}


def dev(x, cuda):
    return torch.from_numpy(np.ascontiguousarray(x)).to(cuda)


def narrow_bytes(rng, shape, fmt):
    """|x| in [0.25, 4) with random signs: all products of two such operands lie within 2^8 of each other."""
    if fmt == E5:
        b = 0x34 + rng.integers(0, 16, size=shape)     # exponents 13..16, both mantissa bits
    else:
        b = 0x28 + rng.integers(0, 0x20, size=shape)   # exponents 5..8, three mantissa bits
    return (b.astype(np.uint8) | (rng.integers(0, 2, size=shape).astype(np.uint8) << 7)).astype(np.uint8)


def run_mm(native, cuda, A, B, sa, sb, fa, fb, *, kernel=L.KERNEL_AUTO, bias=None, scale_result=None, out_dtype=None, split_k=0,
           typed=False, transposed=False, tA=None, tB=None):
    """typed: hand the operands over as float8 tensors (the format comes from the dtype) instead of bytes + a_format / b_format."""
    kw = {}
    if bias is not None:
        kw["bias"] = dev(np.asarray(bias, np.float32), cuda)
    if scale_result is not None:
        kw["scale_result"] = dev(np.array([scale_result], np.float32), cuda)
    tA = dev(A, cuda) if tA is None else tA
    tB = dev(B, cuda) if tB is None else tB
    if typed:
        tA, tB = tA.view(R.TORCH_DTYPE[fa]), tB.view(R.TORCH_DTYPE[fb])
    else:
        kw.update(a_format=fa, b_format=fb)
    got = native.fp8_scaled_mm(tA, tB, dev(np.asarray(sa, np.float32), cuda), dev(np.asarray(sb, np.float32), cuda), out_dtype=out_dtype,
                               kernel=kernel, split_k=split_k, transposed_epilogue=transposed, **kw)
    torch.cuda.synchronize()
    return got


def check(got, A, B, sa, sb, fa, fb, tol, *, bias=None, scale_result=None, out_dtype=None, rms_gate=False, what=""):
    exact, bound = R.mm_ref(A, B, sa, sb, fa, fb, bias=bias, scale_result=scale_result)
    assert got.shape == exact.shape and got.dtype == (out_dtype or torch.float32)
    g = got.float().cpu().numpy().astype(np.float64)
    sr = 1.0 if scale_result is None else abs(float(scale_result))
    babs = 0.0 if bias is None else np.abs(np.asarray(bias, np.float64)).reshape(1, -1) * sr
    allow = tol * bound + 4 * 2.0 ** -24 * (np.abs(exact) + babs) + 1e-30
    if out_dtype in (torch.bfloat16, torch.float16):
        allow = allow + (2.0 ** -8 if out_dtype == torch.bfloat16 else 2.0 ** -11) * np.abs(exact) + (2.0 ** -24 if out_dtype == torch.float16 else 0.0)
    err = np.abs(g - exact)
    ratio = float(np.max(err / (bound + 1e-300)))
    rms = float(np.sqrt(np.mean(err ** 2)) / (np.sqrt(np.mean(bound ** 2)) + 1e-300))
    print(f"[e5m2] {what}: max err/bound {ratio:.3e}  rms err/rms bound {rms:.3e}")
    assert np.all(err <= allow), f"{what}: max err/bound = {ratio:.3e} (tol {tol:.1e})"
    if rms_gate and out_dtype in (None, torch.float32) and g.size >= 64:
        assert rms <= R.MFMA_RMS_TOL, f"{what}: rms err / rms bound = {rms:.3e}"
    return g


# ---------------------------------------------------------------------------------------------------------------------------
# casts
# ---------------------------------------------------------------------------------------------------------------------------

def test_encode_all_f16_and_bf16_bit_patterns(native, cuda):
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    for dt in (torch.float16, torch.bfloat16):
        x = bits.view(dt)
        got = native.fp8_encode_e5m2(x.to(cuda))
        assert got.dtype == torch.float8_e5m2 and got.shape == x.shape
        g, want = got.view(torch.uint8).cpu(), R.encode_ref(x)
        bad = (g != want).nonzero().flatten()
        assert bad.numel() == 0, (dt, [(hex(int(bits[i]) & 0xFFFF), hex(int(g[i])), hex(int(want[i]))) for i in bad[:8]])


def f32_probe_values():
    vals = [0.0, -0.0, 57344.0, -57344.0, 61440.0, -61440.0, 61439.99, 65536.0, 1e9, float("inf"), float("-inf"), float("nan"), -float("nan"),
            2.0 ** -14, 2.0 ** -15, 2.0 ** -16, 2.0 ** -17, 1.5 * 2.0 ** -17, 2.0 ** -18, 1e-30, 1e-45, 3 * 2.0 ** -17, 5 * 2.0 ** -17, 7 * 2.0 ** -17]
    dec = R.DEC_E5M2
    fin = np.sort(np.unique(dec[np.isfinite(dec)]))
    out = list(fin)
    mids = (fin[:-1] + fin[1:]) / 2                              # exact in float32 (a 4-bit significand)
    for m in mids:
        f = np.float32(m)
        out += [f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))]
    return torch.tensor(np.array(vals + out, dtype=np.float32))


def test_encode_f32_values_midpoints_and_specials(native, cuda):
    x = f32_probe_values()
    for off, cnt in ((0, x.numel()), (1, 777), (3, 1001), (5, 1), (16, 64)):   # odd counts, misaligned offsets
        xs = x.to(cuda)[off:off + cnt]
        got = native.fp8_encode_e5m2(xs).view(torch.uint8).cpu()
        want = R.encode_ref(x[off:off + cnt])
        assert torch.equal(got, want), (off, cnt, (got != want).nonzero().flatten()[:8].tolist())
    # with a prescale: the product is rounded to float32 first, as torch's `(x * s).to(float8_e5m2)`
    for s in (0.37, 3.0, 2.0 ** -7, 1e4):
        st = torch.tensor([s], dtype=torch.float32)
        got = native.fp8_encode_e5m2(x.to(cuda), prescale=st.to(cuda)).view(torch.uint8).cpu()
        assert torch.equal(got, R.encode_ref(x * st)), s
    # unaligned raw pointer through the C entry point (a slice of a byte buffer at offset 4)
    buf = torch.zeros(4 + 4 * 333, dtype=torch.uint8, device=cuda)
    src = buf[4:].view(torch.float32)
    src.copy_(x[:333].to(cuda))
    out = torch.empty(333 + 1, dtype=torch.uint8, device=cuda)
    rc = L.load().fp8mi_encode_e5m2(src.data_ptr(), L.F32, out.data_ptr() + 1, None, 333, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(out[1:].cpu(), R.encode_ref(x[:333]))


def test_dequant_all_256_bytes(native, cuda):
    b = torch.arange(256, dtype=torch.int16).to(torch.uint8)
    ref32 = b.view(torch.float8_e5m2).float()
    for src in (b.to(cuda), b.to(cuda).view(torch.float8_e5m2)):
        f = native.fp8_dequantize_e5m2(src, None, out_dtype=torch.float32).cpu()
        assert torch.equal(torch.isnan(f), torch.isnan(ref32)) and torch.equal(f[~torch.isnan(f)].view(torch.int32), ref32[~torch.isnan(ref32)].view(torch.int32))
        h = native.fp8_dequantize_e5m2(src, None, out_dtype=torch.float16).cpu()
        want = (b.to(torch.int16) << 8).view(torch.float16)      # the byte is the high byte of the half
        nn = ~torch.isnan(want)
        assert torch.equal(torch.isnan(h), ~nn) and torch.equal(h[nn].view(torch.int16), want[nn].view(torch.int16))
        bf = native.fp8_dequantize_e5m2(src, None, out_dtype=torch.bfloat16).cpu()
        wbf = ref32.to(torch.bfloat16)
        assert torch.equal(torch.isnan(bf), ~nn) and torch.equal(bf[nn].view(torch.int16), wbf[nn].view(torch.int16))
    # with a scale: cast(float(dec) * scale), the product rounded to fp32 once, then to the output type
    for s in (0.3, 1.0 / 3.0, 1e-3, 7.0):
        st = torch.tensor([s], dtype=torch.float32)
        prod = ref32 * st
        for od in (torch.float32, torch.float16, torch.bfloat16):
            got = native.fp8_dequantize_e5m2(b.to(cuda), st.to(cuda), out_dtype=od).cpu()
            want = prod.to(od)
            nn = ~torch.isnan(want)
            assert torch.equal(torch.isnan(got), ~nn), (s, od)
            assert torch.equal(got[nn].float(), want[nn].float()), (s, od)
            assert torch.equal(torch.signbit(got[nn]), torch.signbit(want[nn])), (s, od)
    z = native.fp8_dequantize_e5m2(torch.zeros(0, dtype=torch.uint8, device=cuda))
    assert z.numel() == 0 and z.dtype == torch.float16


@pytest.mark.parametrize("dt", [torch.float32, torch.float16, torch.bfloat16])
def test_quantize_bytes_and_scales(native, cuda, dt):
    g = torch.Generator().manual_seed(11)
    lib = L.load()
    for n, scale in ((4099, 1.0), (1, 3.0), (65536 + 7, 250.0), (1000, 1e-3)):
        x = (torch.randn(n, generator=g) * scale).to(dt)
        if n > 100:
            x[17] = float("nan")
        q, inv = native.fp8_quantize_e5m2(x.to(cuda))
        wq, wamax, winv = R.quantize_ref(x)
        assert q.dtype == torch.float8_e5m2 and torch.equal(q.view(torch.uint8).cpu(), wq), (n, scale)
        assert inv.cpu().numpy()[0] == winv, (n, scale)
        # both slots of the C entry point's scales
        xs = x.to(cuda)
        out = torch.empty(n, dtype=torch.uint8, device=cuda)
        sc = torch.empty(2, dtype=torch.float32, device=cuda)
        code = {torch.float32: L.F32, torch.float16: L.F16, torch.bfloat16: L.BF16}[dt]
        assert lib.fp8mi_quantize_e5m2(xs.data_ptr(), code, out.data_ptr(), sc.data_ptr(), n, torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        assert sc.cpu().numpy().tolist() == [wamax, winv] and torch.equal(out.cpu(), wq)
    q, inv = native.fp8_quantize_e5m2(torch.zeros(300, dtype=dt, device=cuda))   # all-zero input: scale 1
    assert q.view(torch.uint8).eq(0).all() and inv.item() == 1.0
    # a round trip through the GEMM's scale: dequant(q) * inv is x to e5m2 precision (2 mantissa bits: 2^-3 relative)
    x = torch.randn(4096, generator=g).to(dt)
    q, inv = native.fp8_quantize_e5m2(x.to(cuda))
    back = native.fp8_dequantize_e5m2(q, inv, out_dtype=torch.float32).cpu()
    assert torch.all((back - x.float()).abs() <= 1.001 * 2.0 ** -3 * x.float().abs() + float(inv) * 2.0 ** -16)


# ---------------------------------------------------------------------------------------------------------------------------
# GEMM, exact cases: narrow-range data on every kernel family, MM_TOL
# ---------------------------------------------------------------------------------------------------------------------------

EXACT_CASES = ([(k, 200, 1024, 328) for k in TILE_KERNELS] + [(k, 300, 640, 264) for k in WAVE_KERNELS] +
               [(L.KERNEL_SKINNY, 40, 1152, 200), (L.KERNEL_SKINNY, 9, 384, 50), (L.KERNEL_SKINNY, 64, 4096, 48),
                (L.KERNEL_GEMV, 1, 8192, 300), (L.KERNEL_GEMV, 1, 14336, 512), (L.KERNEL_GEMV, 1, 20480, 96),     # matrix-core vec-mat: three launch forms
                (L.KERNEL_GEMV_MX, 2, 4096, 130), (L.KERNEL_GEMV_MX, 4, 8192, 70), (L.KERNEL_GEMV_MX, 8, 12288, 66), (L.KERNEL_GEMV_MX, 8, 4096, 40),
                (L.KERNEL_GEMV_MX, 6, 8192, 24)])


@pytest.mark.parametrize("fa,fb", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("kernel,M,K,N", EXACT_CASES, ids=[f"{NAMES[c[0]]}-{c[1]}x{c[2]}x{c[3]}" for c in EXACT_CASES])
def test_gemm_exact_on_narrow_range(native, cuda, kernel, M, K, N, fa, fb):
    """Products within 2^8 of each other, asymmetric in m, n and k: the matrix core sums them exactly, so a wrong K-map, a swapped
    cbsz / blgp or a wrong register in the generated loop cannot hide behind the hardware tolerance."""
    rng = np.random.default_rng(1000 * kernel + M + K + N + 7 * fa + 13 * fb)
    A, B = narrow_bytes(rng, (M, K), fa), narrow_bytes(rng, (N, K), fb)
    got = run_mm(native, cuda, A, B, [0.5], [2.0], fa, fb, kernel=kernel, split_k=1)
    check(got, A, B, [0.5], [2.0], fa, fb, R.MM_TOL, what=f"{NAMES[kernel]} narrow {M}x{K}x{N}")


@pytest.mark.parametrize("fa,fb", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("kernel", [L.KERNEL_GEMM_128, L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_256W, L.KERNEL_SKINNY, L.KERNEL_GEMV_MX, L.KERNEL_GENERIC],
                         ids=lambda k: NAMES[k])
def test_gemm_selector_against_random_bytes_is_exact(native, cuda, kernel, fa, fb):
    """One operand selects a row-dependent k with a single 1.0, the other holds random finite bytes of ITS format (values from 2^-16
    to 57344 that decode very differently in the other format): every output is one decoded byte, exactly.  Both orientations - a
    swapped format pair or a k-permutation between the operands shows on its own."""
    M = {L.KERNEL_SKINNY: 48, L.KERNEL_GEMV_MX: 8}.get(kernel, 128)
    N, K = 136, 512
    rng = np.random.default_rng(5 + kernel)
    one = {E4: 0x38, E5: 0x3C}
    # A selects, B random
    A = np.zeros((M, K), np.uint8)
    ka = [(m * 5 + 3) % K for m in range(M)]
    A[np.arange(M), ka] = one[fa]
    B = R.finite_bytes(rng, (N, K), fb)
    got = run_mm(native, cuda, A, B, [1.0], [1.0], fa, fb, kernel=kernel, split_k=1).cpu().numpy()
    assert np.array_equal(got, R.DEC[fb][B][:, ka].T.astype(np.float32)), "A selects"
    # B selects, A random
    B = np.zeros((N, K), np.uint8)
    kb = [(n * 7 + 11) % K for n in range(N)]
    B[np.arange(N), kb] = one[fb]
    A = R.finite_bytes(rng, (M, K), fa)
    got = run_mm(native, cuda, A, B, [1.0], [1.0], fa, fb, kernel=kernel, split_k=1).cpu().numpy()
    assert np.array_equal(got, R.DEC[fa][A][:, kb].astype(np.float32)), "B selects"


def test_mixed_pair_bytes_that_differ_between_the_formats(native, cuda):
    """The same byte matrices multiplied as e5m2 x e4m3 and as e4m3 x e5m2 (bytes 0x30 .. 0x47: 0.125 .. 7 as e5m2, 0.5 .. 3.75 as e4m3;
    products within 2^9 of each other, summed exactly): each equals ITS reference and the two differ - a swap of the operands' format codes would exchange them."""
    rng = np.random.default_rng(42)
    M, K, N = 96, 384, 80
    A = (0x30 + rng.integers(0, 0x18, size=(M, K))).astype(np.uint8)
    B = (0x30 + rng.integers(0, 0x18, size=(N, K))).astype(np.uint8)
    out = {}
    for fa, fb in ((E5, E4), (E4, E5)):
        for kernel in (L.KERNEL_GEMM_128x64, L.KERNEL_GEMM_256x128W, L.KERNEL_SKINNY):
            m = 64 if kernel == L.KERNEL_SKINNY else M
            got = run_mm(native, cuda, A[:m], B, [1.0], [1.0], fa, fb, kernel=kernel, split_k=1)
            out[(fa, fb, kernel)] = check(got, A[:m], B, [1.0], [1.0], fa, fb, R.MM_TOL, what=f"mixed {fa}{fb} {NAMES[kernel]}")
    assert not np.allclose(out[(E5, E4, L.KERNEL_GEMM_128x64)], out[(E4, E5, L.KERNEL_GEMM_128x64)], rtol=1e-2)


# ---------------------------------------------------------------------------------------------------------------------------
# GEMM, random finite bytes
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fa,fb", PAIRS, ids=PAIR_IDS)
def test_gemm_random_bytes_shapes_and_epilogues(native, cuda, fa, fb):
    """Ragged M / N, K tails, split-K, padded strides, rowwise and tensorwise scales, bias, scale_result, all output types, the
    transposed epilogue - on random finite bytes of each operand's format, MFMA_TOL and the rms gate."""
    rng = np.random.default_rng(77 + fa + 2 * fb)
    s = 2.0 ** -14   # e5m2 products reach 3e9: scales that keep sums inside float16
    cases = [  # (kernel, M, K, N, split_k, rowwise, bias, scale_result, out_dtype)
        (L.KERNEL_AUTO, 300, 1040, 200, 0, False, False, None, None),
        (L.KERNEL_AUTO, 512, 4096, 512, 0, True, True, 0.5, torch.bfloat16),
        (L.KERNEL_GEMM_128, 129, 400, 72, 1, True, True, None, torch.float16),
        (L.KERNEL_GEMM_128x64, 257, 2064, 130, 1, False, True, 2.0, None),
        (L.KERNEL_GEMM_256, 300, 656, 264, 1, True, False, None, torch.bfloat16),
        (L.KERNEL_GEMM_64x64, 48, 4096, 256, 4, True, True, None, None),          # forced split-K
        (L.KERNEL_GEMM_32x64, 24, 8192, 192, 0, False, False, 0.25, None),        # the library's own split
        (L.KERNEL_GEMM_64x128, 64, 4112, 384, 3, True, False, None, torch.float16),
        (L.KERNEL_GEMM_32x32, 17, 2048, 100, 2, False, True, None, None),
        (L.KERNEL_GEMM_128D, 200, 768, 328, 1, True, True, 1.5, None),
        (L.KERNEL_GEMM_256W, 300, 656, 264, 1, True, True, 0.5, torch.bfloat16),
        (L.KERNEL_GEMM_256W, 520, 1024, 512, 1, False, False, None, None),
        (L.KERNEL_GEMM_256x128W, 260, 400, 136, 1, False, True, None, torch.float16),
        (L.KERNEL_SKINNY, 33, 2064, 150, 1, True, True, 0.5, None),
        (L.KERNEL_GEMV_MX, 5, 8192, 77, 1, True, True, None, torch.bfloat16),
        (L.KERNEL_GEMV, 1, 8208, 130, 1, True, True, 2.0, None),
        (L.KERNEL_AUTO, 64, 14336, 256, 0, False, False, None, torch.bfloat16),   # decode shape: AUTO splits K
    ]
    for kernel, M, K, N, split, rowwise, has_bias, sr, od in cases:
        A, B = R.finite_bytes(rng, (M, K), fa), R.finite_bytes(rng, (N, K), fb)
        sa = rng.uniform(0.5, 2.0, size=M).astype(np.float32) * np.float32(s) if rowwise else np.array([s], np.float32)
        sb = rng.uniform(0.5, 2.0, size=N).astype(np.float32) * np.float32(s) if rowwise else np.array([s * 1.5], np.float32)
        bias = rng.standard_normal(N).astype(np.float32) if has_bias else None
        got = run_mm(native, cuda, A, B, sa, sb, fa, fb, kernel=kernel, bias=bias, scale_result=sr, out_dtype=od, split_k=split, typed=(M % 2 == 0))
        check(got, A, B, sa, sb, fa, fb, R.MFMA_TOL, bias=bias, scale_result=sr, out_dtype=od, rms_gate=True,
              what=f"{NAMES[kernel]} random {M}x{K}x{N} split {split}")


@pytest.mark.parametrize("fa,fb", PAIRS, ids=PAIR_IDS)
def test_gemm_padded_strides_unaligned_operands_and_transposed_epilogue(native, cuda, fa, fb):
    rng = np.random.default_rng(5 + fa + 2 * fb)
    s = 2.0 ** -14
    # padded row strides (views of wider buffers), no copy
    M, K, N = 130, 1024, 96
    bigA, bigB = R.finite_bytes(rng, (M, K + 256), fa), R.finite_bytes(rng, (N, K + 512), fb)
    A, B = bigA[:, :K], bigB[:, :K]
    for kernel in (L.KERNEL_GEMM_128x64, L.KERNEL_GEMM_256W, L.KERNEL_AUTO):
        got = run_mm(native, cuda, A, B, [s], [s], fa, fb, kernel=kernel, tA=dev(bigA, cuda)[:, :K], tB=dev(bigB, cuda)[:, :K])
        check(got, A, B, [s], [s], fa, fb, R.MFMA_TOL, rms_gate=True, what=f"{NAMES[kernel]} padded strides")
    # K not a multiple of 16: AUTO pads the operands with zero bytes (+0.0 in both formats) and runs a tile kernel
    M, K, N = 64, 200, 512
    A, B = R.finite_bytes(rng, (M, K), fa), R.finite_bytes(rng, (N, K), fb)
    got = run_mm(native, cuda, A, B, [s], [s], fa, fb, typed=True)
    check(got, A, B, [s], [s], fa, fb, R.MFMA_TOL, rms_gate=True, what="padded operands K=200")
    # ... and a small unaligned problem on the generic kernel (fp32 sums of exact products)
    M, K, N = 5, 100, 17
    A, B = R.finite_bytes(rng, (M, K), fa), R.finite_bytes(rng, (N, K), fb)
    got = run_mm(native, cuda, A, B, [s], [s], fa, fb)
    check(got, A, B, [s], [s], fa, fb, R.MM_TOL, what="generic by alignment")
    # transposed epilogue: C^T = W . X^T with bias along the rows and the scales applied in the untransposed order - the bits of
    # the untransposed call, transposed
    M, K, N = 72, 1024, 200
    X, W = R.finite_bytes(rng, (M, K), fa), R.finite_bytes(rng, (N, K), fb)
    sx = rng.uniform(0.5, 2.0, size=M).astype(np.float32) * np.float32(s)
    sw = rng.uniform(0.5, 2.0, size=N).astype(np.float32) * np.float32(s)
    bias = rng.standard_normal(N).astype(np.float32)
    for kernel in (L.KERNEL_GEMM_128, L.KERNEL_GEMM_64x64, L.KERNEL_GEMM_256x128W):
        plain = run_mm(native, cuda, X, W, sx, sw, fa, fb, kernel=kernel, bias=bias, split_k=1)
        tr = run_mm(native, cuda, W, X, sw, sx, fb, fa, kernel=kernel, bias=bias, split_k=1, transposed=True)
        assert torch.equal(tr.t(), plain), NAMES[kernel]
        check(plain, X, W, sx, sw, fa, fb, R.MFMA_TOL, bias=bias, what=f"{NAMES[kernel]} transposed epilogue")


@pytest.mark.parametrize("fa,fb", PAIRS, ids=PAIR_IDS)
def test_fp32_fma_kernels_meet_mm_tol_on_random_bytes(native, cuda, fa, fb):
    """generic, GEMV_FP32 and the vec-mat at K <= 4096 sum exact products in IEEE fp32."""
    rng = np.random.default_rng(9 + fa + 2 * fb)
    s = 2.0 ** -14
    for kernel, M, K, N in ((L.KERNEL_GENERIC, 33, 100, 17), (L.KERNEL_GENERIC, 7, 1023, 65), (L.KERNEL_GENERIC, 64, 512, 64),
                            (L.KERNEL_GEMV_FP32, 1, 4096, 300), (L.KERNEL_GEMV_FP32, 1, 8192, 130), (L.KERNEL_GEMV_FP32, 1, 14336, 70),
                            (L.KERNEL_GEMV_FP32, 1, 20480, 33), (L.KERNEL_GEMV, 1, 4096, 513), (L.KERNEL_GEMV, 1, 1040, 77), (L.KERNEL_AUTO, 1, 2048, 256)):
        A, B = R.finite_bytes(rng, (M, K), fa), R.finite_bytes(rng, (N, K), fb)
        sb = rng.uniform(0.5, 2.0, size=N).astype(np.float32) * np.float32(s)
        bias = rng.standard_normal(N).astype(np.float32)
        got = run_mm(native, cuda, A, B, [s], sb, fa, fb, kernel=kernel, bias=bias, scale_result=0.5)
        check(got, A, B, [s], sb, fa, fb, R.MM_TOL, bias=bias, scale_result=0.5, what=f"{NAMES[kernel]} fp32 {M}x{K}x{N}")


# ---------------------------------------------------------------------------------------------------------------------------
# bits
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fa,fb", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("M,K,N", [(300, 640, 264), (129, 3072, 72)])
def test_every_unsplit_tile_kernel_gives_the_same_bits(native, cuda, M, K, N, fa, fb):
    rng = np.random.default_rng(M + 3 * K + N)
    A, B = R.finite_bytes(rng, (M, K), fa), R.finite_bytes(rng, (N, K), fb)
    sa = rng.uniform(0.5, 2.0, size=M).astype(np.float32) * np.float32(2.0 ** -14)
    sb = rng.uniform(0.5, 2.0, size=N).astype(np.float32) * np.float32(2.0 ** -14)
    bias = rng.standard_normal(N).astype(np.float32)
    for od in (torch.float32, torch.bfloat16):
        ref = None
        for kernel in TILE_KERNELS + WAVE_KERNELS:
            got = run_mm(native, cuda, A, B, sa, sb, fa, fb, kernel=kernel, bias=bias, out_dtype=od, split_k=1)
            ref = got if ref is None else ref
            assert torch.equal(got, ref), (NAMES[kernel], od)
        auto = run_mm(native, cuda, A, B, sa, sb, fa, fb, bias=bias, out_dtype=od, split_k=1)   # AUTO without a K split: one of them
        assert torch.equal(auto, ref), od
        check(ref, A, B, sa, sb, fa, fb, R.MFMA_TOL, bias=bias, out_dtype=od, rms_gate=True, what=f"shared bits {M}x{K}x{N}")


def test_fmt_entry_with_e4m3_formats_is_scaled_mm_ws_bit_for_bit(native, cuda):
    """fp8mi_scaled_mm_fmt(E4M3, E4M3) against fp8mi_scaled_mm_ws through ctypes, NaN bytes and both nan modes included."""
    lib = L.load()
    rng = np.random.default_rng(3)
    stream = torch.cuda.current_stream().cuda_stream
    for kernel, M, K, N in ((L.KERNEL_GEMM_128x64, 200, 1024, 328), (L.KERNEL_GEMM_256W, 300, 640, 264), (L.KERNEL_GEMM_64x64, 64, 4096, 256),
                            (L.KERNEL_SKINNY, 40, 1152, 200), (L.KERNEL_GEMV, 1, 8192, 300), (L.KERNEL_GEMV, 1, 2048, 100), (L.KERNEL_GEMV_MX, 4, 4096, 64),
                            (L.KERNEL_GENERIC, 9, 100, 33), (L.KERNEL_AUTO, 512, 4096, 512)):
        A = rng.integers(0, 256, size=(M, K), dtype=np.uint8)   # NaN bytes included
        B = rng.integers(0, 256, size=(N, K), dtype=np.uint8)
        tA, tB = dev(A, cuda), dev(B, cuda)
        sa, sb = dev(np.array([0.01], np.float32), cuda), dev(rng.uniform(0.005, 0.02, size=N).astype(np.float32), cuda)
        ws = torch.zeros(int(lib.fp8mi_scaled_mm_workspace_bytes()), dtype=torch.uint8, device=cuda)
        for nan_mode in (L.NAN_ZERO, L.NAN_PROPAGATE):
            c1 = torch.empty((M, N), dtype=torch.float32, device=cuda)
            c2 = torch.empty((M, N), dtype=torch.float32, device=cuda)
            head = (sa.data_ptr(), sb.data_ptr(), None, None, M, N, K, K, K, N, L.SCALE_TENSOR, L.SCALE_ROW, L.F32, L.F32, nan_mode, kernel, 0,
                    ws.data_ptr(), ws.numel())
            assert lib.fp8mi_scaled_mm_ws(tA.data_ptr(), tB.data_ptr(), c1.data_ptr(), *head, stream) == 0
            assert lib.fp8mi_scaled_mm_fmt(tA.data_ptr(), tB.data_ptr(), c2.data_ptr(), *head, E4, E4, stream) == 0
            torch.cuda.synchronize()
            assert torch.equal(c1.view(torch.int32), c2.view(torch.int32)), (NAMES[kernel], nan_mode)


# ---------------------------------------------------------------------------------------------------------------------------
# inf / NaN: ordinary IEEE values in known positions
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fa,fb", PAIRS, ids=PAIR_IDS)
def test_inf_and_nan_bytes_propagate_as_ieee(native, cuda, fa, fb):
    """An inf byte (0x7C / 0xFC, in an e5m2 operand) and a NaN byte (0x7F: NaN in both formats) among small magnitudes: the NaN / +inf /
    -inf class of every output equals the float64 reference's (inf * 0 and inf - inf are NaN) on a tile kernel, the one-wave-per-SIMD
    kernel, skinny, both vec-mat forms, the few-rows kernel and the generic one."""
    rng = np.random.default_rng(21 + fa + 2 * fb)
    for kernel, M, K, N in ((L.KERNEL_GEMM_128x64, 130, 640, 100), (L.KERNEL_GEMM_64x64, 64, 2048, 72), (L.KERNEL_GEMM_256W, 260, 512, 136),
                            (L.KERNEL_SKINNY, 20, 512, 90), (L.KERNEL_GEMV, 1, 8192, 64), (L.KERNEL_GEMV, 1, 1024, 64), (L.KERNEL_GEMV_MX, 4, 4096, 40),
                            (L.KERNEL_GENERIC, 6, 200, 30)):
        A, B = narrow_bytes(rng, (M, K), fa), narrow_bytes(rng, (N, K), fb)
        B[:, 5] = np.where(np.arange(N) % 3 == 0, 0, B[:, 5])          # zeros under the inf column: inf * 0
        A[:, 9] = np.where(np.arange(M) % 2 == 0, 0, A[:, 9])
        if fa == E5:
            A[0, 5] = 0x7C                                              # +inf in A: row 0 is +-inf, NaN where B[n, 5] == 0
            if M > 2:
                A[2, 5], A[2, 6] = 0x7C, 0xFC                           # +inf and -inf in one row: inf - inf where both count
        if fb == E5:
            B[1, 9] = 0xFC                                              # -inf in B: column 1
            B[4, 9], B[4, 11] = 0x7C, 0x7C
        B[3, 40] = 0x7F                                                 # NaN byte: column 3
        if M > 5:
            A[5, 77] = 0xFF
        exact, _ = R.mm_ref(A, B, [1.0], [1.0], fa, fb)
        got = run_mm(native, cuda, A, B, [1.0], [1.0], fa, fb, kernel=kernel, split_k=1).cpu().numpy()
        for name, f in (("nan", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
            assert np.array_equal(f(got), f(exact)), (NAMES[kernel], M, K, name, int(f(got).sum()), int(f(exact).sum()))
        assert np.isnan(exact).any()                                    # (the case really holds what it is meant to)
        if M > 1:
            assert np.isinf(exact).any() and np.isfinite(exact).any()
        fin = np.isfinite(exact)
        bound = (np.abs(np.nan_to_num(R.DEC[fa][A], nan=0, posinf=0, neginf=0)) @ np.abs(np.nan_to_num(R.DEC[fb][B], nan=0, posinf=0, neginf=0)).T)
        assert np.all(np.abs(got[fin] - exact[fin]) <= R.MFMA_TOL * bound[fin]), NAMES[kernel]


def test_e5m2_calls_run_with_nan_propagate_whatever_the_module_default(native, cuda):
    assert native.NAN_MODE == L.NAN_ZERO   # the e4m3 default (reference semantics) is untouched ...
    A = np.full((4, 64), 0x3C, np.uint8)
    B = np.full((8, 64), 0x38, np.uint8)
    A[1, 3] = 0x7F
    got = run_mm(native, cuda, A, B, [1.0], [1.0], E5, E4, typed=True).cpu().numpy()   # ... and an e5m2 call propagates
    assert np.isnan(got[1]).all() and np.all(got[[0, 2, 3]] == 64.0)
    lib = L.load()
    tA, tB = dev(A, cuda), dev(B, cuda)
    c = torch.empty((4, 8), device=cuda)
    one = torch.ones(1, device=cuda)
    rc = lib.fp8mi_scaled_mm_fmt(tA.data_ptr(), tB.data_ptr(), c.data_ptr(), one.data_ptr(), one.data_ptr(), None, None, 4, 8, 64, 64, 64, 8,
                                 0, 0, L.F32, L.F32, L.NAN_ZERO, L.KERNEL_AUTO, 1, None, 0, E5, E4, None)
    assert rc == -4


def test_fp8_linear_with_an_e5m2_weight(native, cuda):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 7, 512, generator=g)
    w = torch.randn(256, 512, generator=g) * 0.05
    bias = torch.randn(256, generator=g)
    wq, winv = native.fp8_quantize_e5m2(w.to(cuda))
    want = x @ w.t() + bias
    for weight, kw in ((wq, {}), (wq.view(torch.uint8), {"weight_format": L.FMT_E5M2})):
        y = native.fp8_linear(x.to(cuda), weight, winv, bias=bias.to(cuda), **kw)
        assert y.shape == (3, 7, 256)
        rel = (y.cpu() - want).norm() / want.norm()
        assert rel < 0.12, float(rel)   # e5m2 weights (2 mantissa bits: rms quantisation error ~7 %) x e4m3 activations (~3.5 %)


# ---------------------------------------------------------------------------------------------------------------------------
# the torch._scaled_mm route
# ---------------------------------------------------------------------------------------------------------------------------

class _Counting:
    def __init__(self):
        self.calls = 0

    def __call__(self, *a, **kw):
        self.calls += 1
        return "original"


@pytest.mark.parametrize("fa,fb", PAIRS, ids=PAIR_IDS)
def test_scaled_mm_patch_takes_e5m2_operands(cuda, patch, native, fa, fb):
    rng = np.random.default_rng(31 + fa + 2 * fb)
    M, K, N = 96, 512, 160
    A, B = R.finite_bytes(rng, (M, K), fa), R.finite_bytes(rng, (N, K), fb)
    a = dev(A, cuda).view(R.TORCH_DTYPE[fa])
    b = dev(B, cuda).view(R.TORCH_DTYPE[fb]).t()            # (K, N) column-major, as torch mandates
    s = np.float32(2.0 ** -14)
    sa1, sb1 = torch.tensor([s], device=cuda), torch.tensor([s * 2], device=cuda)
    sar = (torch.rand(M, 1, device=cuda) + 0.5) * float(s)
    sbr = (torch.rand(1, N, device=cuda) + 0.5) * float(s)
    bias = torch.randn(N, device=cuda).to(torch.bfloat16)
    stub = _Counting()
    saved = patch._original_scaled_mm
    patch._original_scaled_mm = stub
    try:
        # keyword scales, float32 (default) result
        got = torch._scaled_mm(a, b, scale_a=sa1, scale_b=sb1)
        check(got, A, B, [s], [s * 2], fa, fb, R.MFMA_TOL, rms_gate=True, what="patch keyword")
        # positional scales, bias, bf16
        got = torch._scaled_mm(a, b, sa1, sb1, bias, None, torch.bfloat16)
        check(got, A, B, [s], [s * 2], fa, fb, R.MFMA_TOL, bias=bias.float().cpu().numpy(), out_dtype=torch.bfloat16, what="patch positional bf16")
        # rowwise scales
        got = torch._scaled_mm(a, b, scale_a=sar, scale_b=sbr, out_dtype=torch.bfloat16)
        check(got, A, B, sar.cpu().numpy(), sbr.cpu().numpy(), fa, fb, R.MFMA_TOL, out_dtype=torch.bfloat16, what="patch rowwise")
        # a float8_e5m2 result: the float32 product through the library's e5m2 cast
        got = torch._scaled_mm(a, b, scale_a=sa1, scale_b=sb1, out_dtype=torch.float8_e5m2)
        assert got.dtype == torch.float8_e5m2
        f32 = torch._scaled_mm(a, b, scale_a=sa1, scale_b=sb1, out_dtype=torch.float32)
        assert torch.equal(got.view(torch.uint8).cpu(), R.encode_ref(f32.cpu()))
        exact, bound = R.mm_ref(A, B, [s], [s * 2], fa, fb)
        assert np.all(np.abs(got.float().cpu().numpy() - exact) <= R.MFMA_TOL * bound + 2.0 ** -3 * np.abs(exact) + 2.0 ** -17)
        # a row-major `other` (not the layout torch mandates): the general entry copies and still knows the formats
        got = torch._scaled_mm(a, dev(np.ascontiguousarray(B.T), cuda).view(R.TORCH_DTYPE[fb]), scale_a=sa1, scale_b=sb1)
        check(got, A, B, [s], [s * 2], fa, fb, R.MFMA_TOL, what="patch row-major other")
        assert stub.calls == 0, "an e5m2 call with float scales reached torch's own _scaled_mm"
        # E8M0 scales and blockwise-shaped scales next to an e5m2 operand: torch's own op, as before
        e8a = torch.full((128, 16), 127, dtype=torch.uint8, device=cuda).view(torch.float8_e8m0fnu)
        e8b = torch.full((256, 16), 127, dtype=torch.uint8, device=cuda).view(torch.float8_e8m0fnu)
        assert torch._scaled_mm(a, b, scale_a=e8a, scale_b=e8b, out_dtype=torch.bfloat16) == "original" and stub.calls == 1
        assert torch._scaled_mm(a, b, scale_a=torch.ones(M, K // 128, device=cuda), scale_b=torch.ones(K // 128, (N + 127) // 128, device=cuda),
                                out_dtype=torch.bfloat16) == "original" and stub.calls == 2
    finally:
        patch._original_scaled_mm = saved


def test_uninstall_restores_the_original_objects(cuda):
    import fp8_mps_patch
    before = (torch._scaled_mm, torch.Tensor.to, torch.Tensor.copy_)
    fp8_mps_patch.install()
    assert torch._scaled_mm is fp8_mps_patch._metal_scaled_mm
    a = torch.zeros(16, 64, dtype=torch.uint8, device=cuda).view(torch.float8_e5m2)
    b = torch.zeros(32, 64, dtype=torch.uint8, device=cuda).view(torch.float8_e5m2).t()
    one = torch.ones(1, device=cuda)
    assert torch._scaled_mm(a, b, scale_a=one, scale_b=one).eq(0).all()
    fp8_mps_patch.uninstall()
    assert (torch._scaled_mm, torch.Tensor.to, torch.Tensor.copy_) == before and not fp8_mps_patch.is_installed()


# ---------------------------------------------------------------------------------------------------------------------------
# C ABI from a plain C host
# ---------------------------------------------------------------------------------------------------------------------------

def test_c_abi_e5m2_roundtrip_without_torch(cuda, tmp_path):
    exe = str(tmp_path / "e5m2_roundtrip")
    cmd = ["gcc", "-O2", "-D__HIP_PLATFORM_AMD__", os.path.join(ROOT, "tests", "c", "e5m2_roundtrip.c"), "-I/opt/rocm/include",
           "-I" + os.path.join(ROOT, "include"), "-L" + PKG, "-lfp8mi", "-L/opt/rocm/lib", "-lamdhip64", "-lm",
           "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "e5m2 C ABI round trip: ok" in out.stdout
