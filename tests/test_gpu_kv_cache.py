"""fp8mi_kv_cache_append on the GPU: the bytes it stores equal fp8mi_encode's of the same values with prescale = 1.0f / scale, byte for
byte, in both cache layouts (K [num_blocks, Hkv, block_size, D], V [num_blocks, Hkv, D, block_size]); every other byte of both caches
keeps its sentinel, as do the guard elements around them; one launch.  Shapes are the smallest that cover the kernel's index arithmetic:
T 1, 3 and 65 (more than one workgroup at Hkv 8), Hkv 1 and 8 (3 and 5 at T 7: no powers of two), both head dimensions, every block
size, the three input dtypes, both scale modes, both slot widths, both encode modes, k and v as strided slices of one qkv tensor."""
import pytest
import torch

import fp8_mi355x_lib as L
from moe_route_gpu_util import DEV, SENT_B, guarded, guards_intact, stream

pytestmark = pytest.mark.gpu

CODE = {torch.float32: L.F32, torch.float16: L.F16, torch.bfloat16: L.BF16}
DTYPES = (torch.float32, torch.float16, torch.bfloat16)


@pytest.fixture(scope="module")
def lib():
    return L.load()


def encode_heads(lib, x, scale, enc):
    """fp8mi_encode of x (T, Hkv, D), head by head, with prescale = 1.0f / scale_h (divided on the CPU: IEEE) -> uint8 (T, Hkv, D) on the CPU"""
    T, Hkv, D = x.shape
    out = torch.empty((Hkv, T, D), dtype=torch.uint8, device=DEV)
    for h in range(Hkv):
        src = x[:, h, :].contiguous()
        pre = (torch.ones(1) / scale[h if scale.numel() > 1 else 0].reshape(1)).to(DEV)
        L.check(lib.fp8mi_encode(src.data_ptr(), CODE[x.dtype], out[h].data_ptr(), pre.data_ptr(), src.numel(), enc, stream()), "fp8mi_encode")
    torch.cuda.synchronize()
    return out.permute(1, 0, 2).cpu()


def run_append(lib, k, v, nb, bs, slots, ks, vs, enc, caches=None):
    """-> (K cache, V cache) on the CPU after one fp8mi_kv_cache_append into caches prefilled with the sentinel; guards checked, one launch"""
    T, Hkv, D = k.shape
    n = nb * Hkv * bs * D
    if caches is None:
        caches = guarded(n, torch.uint8, SENT_B), guarded(n, torch.uint8, SENT_B)
    (kbuf, kc), (vbuf, vc) = caches
    ks_d, vs_d = ks.to(DEV), vs.to(DEV)
    with L.kernel_timer(4) as kt:
        rc = lib.fp8mi_kv_cache_append(k.data_ptr(), v.data_ptr(), CODE[k.dtype], T, Hkv, D, k.stride(0) if T > 1 else Hkv * D,
                                       v.stride(0) if T > 1 else Hkv * D, kc.data_ptr(), vc.data_ptr(), nb, bs, slots.data_ptr(), slots.element_size(),
                                       ks_d.data_ptr(), vs_d.data_ptr(), L.KV_SCALE_HEAD if ks.numel() > 1 else L.KV_SCALE_TENSOR, enc, stream())
    L.check(rc, "fp8mi_kv_cache_append")
    torch.cuda.synchronize()
    assert len(kt.ms) == 1
    assert guards_intact(kbuf, n, SENT_B) and guards_intact(vbuf, n, SENT_B)
    return kc.reshape(nb, Hkv, bs, D).cpu(), vc.reshape(nb, Hkv, D, bs).cpu()


def expected_caches(lib, k, v, nb, bs, slots, ks, vs, enc):
    T, Hkv, D = k.shape
    want_k = torch.full((nb, Hkv, bs, D), SENT_B, dtype=torch.uint8)
    want_v = torch.full((nb, Hkv, D, bs), SENT_B, dtype=torch.uint8)
    ek, ev = encode_heads(lib, k, ks, enc), encode_heads(lib, v, vs, enc)
    for t, slot in enumerate(slots.cpu().tolist()):
        if 0 <= slot < nb * bs:
            want_k[slot // bs, :, slot % bs, :] = ek[t]
            want_v[slot // bs, :, :, slot % bs] = ev[t]
    return want_k, want_v


def qkv_slices(gen, T, Hkv, D, dtype, amp=1.0):
    """k and v as strided slices of one fused (T, (4 + 2) Hkv D) tensor"""
    qkv = (amp * torch.randn((T, 6 * Hkv * D), generator=gen)).to(dtype).to(DEV)
    k = qkv[:, 4 * Hkv * D:5 * Hkv * D].view(T, Hkv, D)
    v = qkv[:, 5 * Hkv * D:].view(T, Hkv, D)
    assert T == 1 or (k.stride(0) == 6 * Hkv * D and not k.is_contiguous())   # (one token: its row stride is never used)
    return k, v


def scattered_slots(gen, T, nb, bs, dtype):
    """T distinct slots over non-adjacent blocks, in a non-monotonic order"""
    while True:
        slots = torch.randperm(nb * bs, generator=gen)[:T]
        up = slots[1:] > slots[:-1]
        if T <= 2 or (bool(up.any()) and not bool(up.all()) and len(set((slots // bs).tolist())) > 1):
            return slots.to(dtype).to(DEV)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("D", (64, 128))
@pytest.mark.parametrize("bs", (16, 32, 64, 128))
def test_append_is_byte_equal_to_encode(lib, bs, D, dtype):
    gen = torch.Generator().manual_seed(100 * bs + D)
    i = 0
    for T in (1, 3, 65):
        for Hkv in (1, 8):
            for per_head in (False, True):
                nb = (T + bs - 1) // bs + 3
                k, v = qkv_slices(gen, T, Hkv, D, dtype, amp=2.0)
                n_s = Hkv if per_head else 1
                ks, vs = 0.004 + 0.01 * torch.rand(n_s, generator=gen), 0.004 + 0.01 * torch.rand(n_s, generator=gen)   # 2 / 0.004 = 500: some values saturate
                slots = scattered_slots(gen, T, nb, bs, (torch.int32, torch.int64)[i % 2])
                enc = (L.ENC_REFERENCE, L.ENC_RNE)[(i // 2) % 2]
                i += 1
                got_k, got_v = run_append(lib, k, v, nb, bs, slots, ks, vs, enc)
                want_k, want_v = expected_caches(lib, k, v, nb, bs, slots, ks, vs, enc)
                what = (T, Hkv, per_head, enc, slots.dtype)
                assert torch.equal(got_k, want_k), what
                assert torch.equal(got_v, want_v), what


@pytest.mark.parametrize("Hkv", (3, 5))
def test_append_with_a_head_count_that_is_no_power_of_two(lib, Hkv):
    """idx -> (token, head, 4 channels) divides by Hkv D / 4: 7 tokens (more than one workgroup at D = 128), both layouts, both scale
    modes, both slot widths"""
    gen = torch.Generator().manual_seed(300 + Hkv)
    T = 7
    for i, (bs, D) in enumerate(((16, 128), (64, 64), (128, 128), (32, 64))):
        nb = 4
        k, v = qkv_slices(gen, T, Hkv, D, DTYPES[i % 3], amp=2.0)
        n_s = Hkv if i % 2 else 1
        ks, vs = 0.004 + 0.01 * torch.rand(n_s, generator=gen), 0.004 + 0.01 * torch.rand(n_s, generator=gen)
        slots = scattered_slots(gen, T, nb, bs, (torch.int32, torch.int64)[(i // 2) % 2])
        got_k, got_v = run_append(lib, k, v, nb, bs, slots, ks, vs, L.ENC_RNE)
        want_k, want_v = expected_caches(lib, k, v, nb, bs, slots, ks, vs, L.ENC_RNE)
        assert torch.equal(got_k, want_k) and torch.equal(got_v, want_v), (Hkv, bs, D)


def test_contiguous_inputs_and_single_token_strides(lib):
    gen = torch.Generator().manual_seed(7)
    for T in (1, 5):
        k = torch.randn((T, 2, 64), generator=gen).to(DEV)
        v = torch.randn((T, 2, 64), generator=gen).to(DEV)
        s = torch.tensor([0.01])
        slots = scattered_slots(gen, T, 4, 16, torch.int64)
        got = run_append(lib, k, v, 4, 16, slots, s, s, L.ENC_RNE)
        want = expected_caches(lib, k, v, 4, 16, slots, s, s, L.ENC_RNE)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_negative_and_out_of_range_slots_store_nothing(lib):
    gen = torch.Generator().manual_seed(11)
    T, Hkv, D, nb, bs = 9, 2, 128, 3, 32
    k, v = qkv_slices(gen, T, Hkv, D, torch.bfloat16)
    s = torch.tensor([0.01])
    # every slot padding: both caches bit-identical to what they held
    for slots in (torch.full((T,), -1), torch.tensor([-1, -5, -(1 << 40), nb * bs, nb * bs + 7, 1 << 40, -1, -2, -3])):
        got_k, got_v = run_append(lib, k, v, nb, bs, slots.to(DEV), s, s, L.ENC_RNE)
        assert bool((got_k == SENT_B).all()) and bool((got_v == SENT_B).all())
    # padding mixed with real slots, int32
    slots = torch.tensor([5, -1, 70, -1, 2, 95, -7, 33, 0], dtype=torch.int32).to(DEV)
    got = run_append(lib, k, v, nb, bs, slots, s, s, L.ENC_REFERENCE)
    want = expected_caches(lib, k, v, nb, bs, slots, s, s, L.ENC_REFERENCE)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert int((got[0] != SENT_B).any(dim=3).any(dim=1).sum()) <= 6   # six positions written, at most


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_range_ends_saturate_or_become_nan_as_encode_does(lib, dtype):
    """The float range's ends, the saturation boundary on both sides, the subnormal and flush boundaries, signed zeros, infinities and NaN,
    in both encode modes and under scales that move them across the boundaries."""
    fmax = torch.finfo(dtype).max
    tiny = torch.finfo(dtype).tiny
    vals = [0.0, -0.0, 1.0, -1.0, 447.9, 448.0, 448.1, 463.9, 464.0, 464.1, 480.0, -448.0, -464.0, -465.0, 2.0 ** -9, 2.0 ** -10, 2.0 ** -10 * 1.01,
            2.0 ** -6, 1.9375, 1.97, 0.0155, fmax, -fmax, tiny, -tiny, float("inf"), float("-inf"), float("nan"), 3.0e4, -6.5e4, 1e-30, 240.0]
    D, Hkv = 64, 2
    T = (len(vals) + D * Hkv - 1) // (D * Hkv) + 1
    x = torch.tensor(vals + [0.5] * (T * Hkv * D - len(vals))).reshape(T, Hkv, D).to(dtype).to(DEV)
    y = x.flip(0).contiguous()
    slots = torch.tensor([17, 3][:T] if T <= 2 else list(range(T))).to(DEV)
    for scale in (torch.tensor([1.0]), torch.tensor([0.5, 2.0]), torch.tensor([1e-30, 1e30]), torch.tensor([3.0])):
        for enc in (L.ENC_REFERENCE, L.ENC_RNE):
            got = run_append(lib, x, y, 2, 16, slots, scale, scale.flip(0), enc)
            want = expected_caches(lib, x, y, 2, 16, slots, scale, scale.flip(0), enc)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (scale.tolist(), enc)
    # and the bytes themselves where the definition is short: RNE mode, scale 1
    got_k, _ = run_append(lib, x, y, 2, 16, slots, torch.tensor([1.0]), torch.tensor([1.0]), L.ENC_RNE)
    row = got_k[int(slots[0]) // 16, :, int(slots[0]) % 16, :].reshape(-1)
    at = {v: i for i, v in enumerate(vals) if v == v}
    assert row[at[448.0]] == 0x7E and row[at[-448.0]] == 0xFE and row[at[480.0]] == 0x7F and row[at[float("inf")]] == 0x7F and row[at[1.0]] == 0x38
    assert row[len(vals) - 5] & 0x7F == 0x7F   # the NaN, with whatever sign bit the input's NaN carries
