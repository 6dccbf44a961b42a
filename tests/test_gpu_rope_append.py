"""fp8mi_rope_kv_cache_append and fp8mi_mla_rope_cache_append on the GPU, through the op layer.  Without a norm everything is held to the
bit: the cache bytes equal the existing append entry run on rope_ref.rotate32's float32 output (and on v), q_out equals rotate32(q) rounded to
its dtype, the contiguous copies equal the bytes at the slots; every other byte keeps its sentinel, the guards too; one launch.  T 1, 3 and 37
take the wave-per-rows kernel, 69 (four full 16-token tiles and a ragged one, ten workgroups) the tiled one; slots in an aligned run (the
transposed V stores), a run from an odd slot across block boundaries and a scattered order.  With a norm: the tolerances of the issue, stated
at the assertions."""
import numpy as np
import pytest
import torch

import fp8_mi355x_lib as L
import fp8_mi355x_native as N
import rope_ref as R
from moe_route_gpu_util import DEV, SENT_B, SENT_F, bits, guarded, guards_intact

pytestmark = pytest.mark.gpu

DTYPES = (torch.float32, torch.float16, torch.bfloat16)
MAX_POS = 40
U = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


def table(gen, rot_dim, dtype):
    ang = torch.rand((MAX_POS, rot_dim // 2), generator=gen) * 6.3
    return torch.cat([ang.cos(), ang.sin()], dim=1).to(dtype).to(DEV)


def fused(gen, T, widths, dtype, skew=0):
    """one (T, sum(widths) + pad) tensor and its column slices: rows with a stride of their own, shifted by `skew` elements"""
    x = (2 * torch.randn((T, sum(widths) + 8 + skew), generator=gen)).to(dtype).to(DEV)
    out, at = [], skew
    for w in widths:
        out.append(x[:, at:at + w])
        at += w
    return out


def slots_of(gen, pattern, T, nb, bs, dtype):
    if pattern == "run":
        s = 16 + torch.arange(T)
    elif pattern == "odd":
        s = bs - 3 + torch.arange(T)
    else:
        s = torch.randperm(nb * bs, generator=gen)[:T]
    return s.to(dtype).to(DEV)


def check_kv(gen, dtype, D, style, T, pattern, i, skew=0, rot_dim=None, pos=None, slots=None):
    """one call against the existing append on rotate32; i picks the other parameters"""
    rot_dim = (D, D // 2)[i % 2] if rot_dim is None else rot_dim
    enc, (Hq, Hkv), bs = (L.ENC_REFERENCE, L.ENC_RNE)[i // 2 % 2], ((4, 1), (6, 3))[i // 3 % 2], (16, 128)[(i + i // 4) % 2]
    idx = ((torch.int32, torch.int64), (torch.int64, torch.int32), (torch.int64, torch.int64), (torch.int32, torch.int32))[i % 4]
    in_place, per_head, cs = i % 3 != 0, i % 5 == 0, table(gen, rot_dim, DTYPES[(i + 1) % 3])
    nb = (T + 16) // bs + 3
    q, k, v = (x.view(T, -1, D) for x in fused(gen, T, (Hq * D, Hkv * D, Hkv * D), dtype, skew))
    pos = torch.randint(0, MAX_POS, (T,), generator=gen) if pos is None else pos
    slots = slots_of(gen, pattern, T, nb, bs, idx[1]) if slots is None else slots(nb * bs).to(DEV)   # (given: a function of the cache's slot count)
    ks, vs = (0.004 + 0.01 * torch.rand(Hkv if per_head else 1, generator=gen) for _ in range(2))   # 2 / 0.004 = 500: some values saturate
    n = nb * Hkv * bs * D
    (kbuf, kc), (vbuf, vc) = guarded(n, torch.uint8, SENT_B), guarded(n, torch.uint8, SENT_B)
    (k8buf, k8), (v8buf, v8) = guarded(T * Hkv * D, torch.uint8, SENT_B), guarded(T * Hkv * D, torch.uint8, SENT_B)
    qbuf, qo = guarded(T * Hq * D, dtype, SENT_F)
    q0 = q.clone()
    with L.kernel_timer(4) as kt:
        got = N.fp8_rope_kv_cache_append(q, k, v, pos.to(idx[0]).to(DEV), cs, kc.view(nb, Hkv, bs, D), vc.view(nb, Hkv, D, bs), slots, ks, vs, rot_dim=rot_dim,
                                         style=style, q_out=None if in_place else qo.view(T, Hq, D), k8_out=k8.view(T, Hkv, D), v8_out=v8.view(T, Hkv, D),
                                         encode_mode=enc)
    torch.cuda.synchronize()
    what = (T, pattern, i, rot_dim)
    assert len(kt.ms) == 1 and all(guards_intact(b, c, f) for b, c, f in ((kbuf, n, SENT_B), (vbuf, n, SENT_B), (k8buf, k8.numel(), SENT_B), (v8buf, v8.numel(), SENT_B),
                                                                         (qbuf, qo.numel(), SENT_F))), what
    ok = ((pos >= 0) & (pos < MAX_POS))
    safe = pos.clamp(0, MAX_POS - 1)
    yq, yk = R.rotate32(q0, cs, safe, rot_dim, style), R.rotate32(k, cs, safe, rot_dim, style)
    want_q = torch.where(ok[:, None, None], yq.to(dtype), q0.cpu() if in_place else torch.full_like(yq, SENT_F).to(dtype))
    assert torch.equal(bits(got[0].cpu()), bits(want_q)), what
    # the existing entries on y: the caches (a token without a valid position gets no slot), the contiguous bytes
    (_, rkc), (_, rvc) = guarded(n, torch.uint8, SENT_B), guarded(n, torch.uint8, SENT_B)
    N.fp8_kv_cache_append(yk.to(DEV), v.float(), rkc.view(nb, Hkv, bs, D), rvc.view(nb, Hkv, D, bs), torch.where(ok.to(DEV), slots.long(), -1), ks, vs, encode_mode=enc)
    assert torch.equal(kc, rkc) and torch.equal(vc, rvc), what
    for mine, x, s in ((got[1], yk, ks), (got[2], v.float(), vs)):
        want = torch.where(ok[:, None, None], N.fp8_attention_kv_quantize(x.to(DEV), s, encode_mode=enc).cpu(), torch.tensor(SENT_B, dtype=torch.uint8))
        assert torch.equal(mine.cpu(), want), what
    live = ok & (slots.cpu() >= 0) & (slots.cpu() < nb * bs)
    at = slots.cpu().long()[live]
    assert torch.equal(kc.view(nb, Hkv, bs, D).cpu()[at // bs, :, at % bs], got[1].cpu()[live]), what
    assert torch.equal(vc.view(nb, Hkv, D, bs).cpu()[at // bs, :, :, at % bs], got[2].cpu()[live]), what


@pytest.mark.parametrize("style", ("neox", "gptj"))
@pytest.mark.parametrize("D", (64, 128))
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_cache_bytes_and_q_out_equal_the_existing_append_on_rotate32(dtype, D, style):
    gen = torch.Generator().manual_seed(D + len(style))
    i = DTYPES.index(dtype) + D // 64
    for T in (1, 3, 37, 69):
        for pattern in ("run", "odd", "scattered"):
            check_kv(gen, dtype, D, style, T, pattern, i)
            i += 1
    # the scalar form: bases and strides that are no multiple of 16 bytes, and a rotary half of an odd number of quads (one lane then holds
    # rotary and pass-through quads)
    for T, pattern, skew, rot_dim in ((3, "odd", 2, D), (69, "run", 0, D // 2 - 8), (37, "scattered", 1, D - 8), (69, "run", 2, 8)):
        check_kv(gen, dtype, D, style, T, pattern, i, skew=skew, rot_dim=rot_dim)
        i += 1


@pytest.mark.parametrize("T", (5, 69))
def test_padding_positions_write_nothing_and_padding_slots_no_cache_byte(T):
    gen = torch.Generator().manual_seed(T)
    pos = torch.randint(0, MAX_POS, (T,), generator=gen)
    pos[0], pos[T - 2] = -1, MAX_POS

    def slots(end):   # -1, the first slot past the cache and one beyond it, at valid positions: q_out and the copies are written, the caches are not
        s = 16 + torch.arange(T)
        s[1], s[2], s[T - 1] = -1, end + 7, end
        return s

    for i, style in enumerate(("neox", "gptj")):
        check_kv(gen, torch.bfloat16, 128, style, T, "given", 4 + i, pos=pos, slots=slots)
    # no q, no caches: the copies alone
    k, v = (x.view(T, 2, 64) for x in fused(gen, T, (128, 128), torch.float16))
    cs = table(gen, 64, torch.float32)
    _, k8, v8 = N.fp8_rope_kv_cache_append(None, k, v, pos.clamp(0, MAX_POS - 1), cs, None, None, None, 0.01, 0.02, k8_out=True, v8_out=True, encode_mode=L.ENC_RNE)
    yk = R.rotate32(k, cs, pos.clamp(0, MAX_POS - 1), 64, "neox")
    assert torch.equal(k8, N.fp8_attention_kv_quantize(yk.to(DEV), 0.01, encode_mode=L.ENC_RNE)) and torch.equal(v8, N.fp8_attention_kv_quantize(v, 0.02, encode_mode=L.ENC_RNE))


def run_mla(gen, dtype, style, T, Hq, i, kvw=None, scale=0.01):
    enc, bs = (L.ENC_REFERENCE, L.ENC_RNE)[i % 2] if kvw is None else L.ENC_RNE, (16, 64)[i // 2 % 2]
    nb = T // bs + 3
    kv_c, k_pe, q_pe = fused(gen, T, (512, 64, Hq * 64), dtype)
    q_pe = q_pe.view(T, Hq, 64) if Hq else None
    cs = table(gen, 64, DTYPES[i % 3])
    pos = torch.randint(0, MAX_POS, (T,), generator=gen)
    slots = slots_of(gen, ("run", "scattered")[i % 2], T, nb, bs, (torch.int32, torch.int64)[i % 2])
    if T > 2 and kvw is None:
        pos[1], slots[2], slots[0] = MAX_POS + 3, -1, nb * bs   # (the first slot past the cache)
    cbuf, cache = guarded(nb * bs * 576, torch.uint8, SENT_B)
    q0 = q_pe.clone() if Hq else None
    with L.kernel_timer(4) as kt:
        got = N.fp8_mla_rope_cache_append(kv_c, k_pe, q_pe, pos.to((torch.int64, torch.int32)[i % 2]).to(DEV), cs, cache.view(nb, bs, 576), slots, scale, style=style,
                                          kv_weight=kvw, encode_mode=enc)
    torch.cuda.synchronize()
    assert len(kt.ms) == 1 and guards_intact(cbuf, cache.numel(), SENT_B) and got is q_pe   # (in place)
    return kv_c, k_pe, q0, got, cs, pos, slots, cache.view(nb, bs, 576), enc


@pytest.mark.parametrize("style", ("neox", "gptj"))
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_mla_rows_equal_the_existing_append_on_rotate32(dtype, style):
    gen = torch.Generator().manual_seed(len(style))
    for i, (T, Hq) in enumerate(((1, 128), (3, 5), (37, 16), (37, 0))):
        kv_c, k_pe, q0, got, cs, pos, slots, cache, enc = run_mla(gen, dtype, style, T, Hq, i + DTYPES.index(dtype))
        ok, safe = pos < MAX_POS, pos.clamp(0, MAX_POS - 1)
        if Hq:
            want_q = torch.where(ok[:, None, None], R.rotate32(q0, cs, safe, 64, style).to(dtype), q0.cpu())
            assert torch.equal(bits(got.cpu()), bits(want_q)), (T, Hq)
        (_, ref) = guarded(cache.numel(), torch.uint8, SENT_B)
        N.fp8_mla_cache_append(kv_c.float(), R.rotate32(k_pe[:, None], cs, safe, 64, style)[:, 0].to(DEV), ref.view(cache.shape), torch.where(ok.to(DEV), slots.long(), -1),
                               0.01, encode_mode=enc)
        assert torch.equal(cache.reshape(-1), ref), (T, Hq)


def within_fp8(byte_rows, r):
    """every byte decodes to within half an e4m3 ulp of r plus the float32 budget 2^-14 |r| (a sum of at most 512 squares in any order is
    512 2^-24 = 2^-15 relative, plus the rsqrt and four roundings)"""
    assert np.abs(r).max() < 448
    ulp8 = np.maximum(2.0 ** (np.floor(np.log2(np.maximum(np.abs(r), 1e-300))) - 3), 2.0 ** -9)
    return bool((np.abs(byte_rows.cpu().view(torch.float8_e4m3fn).double().numpy() - r) <= 0.5 * ulp8 + 2.0 ** -14 * np.abs(r)).all())


@pytest.mark.parametrize("D", (64, 128))
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_q_and_k_norm_within_the_float32_budget(dtype, D):
    gen = torch.Generator().manual_seed(D)
    for T, style in ((3, "neox"), (69, "gptj")):
        Hq, Hkv, scale = 6, 3, 0.05   # |n| stays below 4.5 sigma x 1.8 x sqrt(2): |r| < 448 with room
        q, k, v = (x.view(T, -1, D) for x in fused(gen, T, (Hq * D, Hkv * D, Hkv * D), dtype))
        qw, kw = (1 + 0.2 * torch.randn(D, generator=gen)).to(DEV), (1 + 0.2 * torch.randn(D, generator=gen)).to(DEV)
        cs, pos = table(gen, D // 2, torch.float32), torch.randint(0, MAX_POS, (T,), generator=gen)
        qo = torch.empty((T, Hq, D), dtype=dtype, device=DEV)
        _, k8, _ = N.fp8_rope_kv_cache_append(q, k, v, pos, cs, None, None, None, scale, scale, style=style, q_weight=qw, k_weight=kw, eps=1e-5, q_out=qo, k8_out=True,
                                              encode_mode=L.ENC_RNE)
        yq, mag = R.rotate64(q, cs, pos, D // 2, style, qw, 1e-5)
        assert bool((np.abs(qo.cpu().double().numpy() - yq) <= (2.0 ** -14 + U[dtype]) * mag).all()), (T, style)
        assert within_fp8(k8, R.rotate64(k, cs, pos, D // 2, style, kw, 1e-5)[0] / scale), (T, style)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_mla_latent_norm_within_the_float32_budget(dtype):
    gen = torch.Generator().manual_seed(9)
    kvw = (1 + 0.2 * torch.randn(512, generator=gen)).to(DEV)
    kv_c, _k_pe, _q0, _got, _cs, _pos, slots, cache, _enc = run_mla(gen, dtype, "gptj", 37, 4, 1, kvw=kvw, scale=0.05)
    n = kv_c.double().cpu().numpy()
    n = n / np.sqrt((n * n).mean(axis=-1, keepdims=True) + 1e-6) * kvw.double().cpu().numpy()
    assert within_fp8(cache.reshape(-1, 576)[slots.long(), :512], n / 0.05)


def test_a_captured_call_replays_on_new_positions_and_slots():
    gen = torch.Generator().manual_seed(3)
    T, Hq, Hkv, D, nb, bs = 69, 4, 2, 128, 8, 16
    q, k, v = (x.view(T, -1, D) for x in fused(gen, T, (Hq * D, Hkv * D, Hkv * D), torch.bfloat16))
    cs = table(gen, D, torch.float32)
    kc, vc = N.fp8_kv_cache_alloc(nb, bs, Hkv, D, device=DEV)
    qo, pos, slots = torch.empty((T, Hq, D), dtype=torch.bfloat16, device=DEV), torch.zeros(T, dtype=torch.int64, device=DEV), torch.arange(T, device=DEV)
    s = torch.full((1,), 0.01, device=DEV)
    call = lambda kc_, vc_, qo_: N.fp8_rope_kv_cache_append(q, k, v, pos, cs, kc_, vc_, slots, s, s, q_out=qo_, encode_mode=L.ENC_RNE)   # noqa: E731
    call(kc, vc, qo)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call(kc, vc, qo)
    for new_slots in (16 + torch.arange(T), torch.randperm(nb * bs, generator=gen)[:T]):
        pos.copy_(torch.randint(0, MAX_POS, (T,), generator=gen))
        slots.copy_(new_slots)
        for _ in range(2):
            kc.zero_(), vc.zero_(), qo.zero_()
            g.replay()
        ekc, evc = N.fp8_kv_cache_alloc(nb, bs, Hkv, D, device=DEV)
        eq = torch.empty_like(qo)
        call(ekc, evc, eq)
        torch.cuda.synchronize()
        assert torch.equal(kc, ekc) and torch.equal(vc, evc) and torch.equal(bits(qo), bits(eq))
