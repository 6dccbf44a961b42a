"""fp8mi_attention_prefill / fp8_attention / fp8_sdpa / fp8_attention_kv_quantize on the GPU: every element within
TOL_flash max|V| of the float64 reference of the expansion; isolation; the argument checks; the producer's bytes; graph replay."""
import numpy as np
import pytest
import torch

import fp8_mi355x_lib as L
import flash_attn_ref as F
import paged_attn_ref as R
from moe_route_gpu_util import CODE, DEV, SENT_F, bits, stream

pytestmark = pytest.mark.gpu
TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
E_NULL, E_SHAPE, E_ENUM, E_UNSUPPORTED = -1, -2, -3, -4   # include/fp8mi.h


@pytest.fixture(scope="module")
def lib():
    return L.load()


@pytest.fixture(scope="module")
def N_():
    import fp8_mi355x_native as N
    return N


class Device:
    """a case's tensors on the device; extra_k: junk-free spare key rows behind cu_k[B]; extra_q: output rows nobody owns.  A `fused` case takes q
    from a wider row and k, v from one (Tk, Hkv, 2, 128) buffer: strided, read in place"""

    def __init__(self, c, extra_k=0, extra_q=0):
        T, Hq, DQK = c.q.shape
        Tk, pad = c.k.shape[0] + extra_k, 64 if c.fused else 0
        self.T, self.Tk = T + extra_q, Tk
        q = torch.zeros((self.T, Hq * DQK + pad), dtype=TORCH[c.q_dtype])
        q[:T, :Hq * DQK] = torch.from_numpy(c.q).reshape(T, -1).to(q.dtype)
        self.q = q.to(DEV)
        kv = torch.zeros((Tk, c.Hkv, 2, F.DV), dtype=torch.uint8)
        kv[:c.k.shape[0], :, 0], kv[:c.k.shape[0], :, 1] = torch.from_numpy(c.k), torch.from_numpy(c.v)
        kv = kv.to(DEV)
        self.k, self.v = (kv[:, :, 0], kv[:, :, 1]) if c.fused else (kv[:, :, 0].contiguous(), kv[:, :, 1].contiguous())
        self.kr = None
        if c.k_rope is not None:
            self.kr = torch.zeros((Tk, c.Hr, F.ROPE), dtype=torch.uint8)
            self.kr[:c.k.shape[0]] = torch.from_numpy(c.k_rope)
            self.kr = self.kr.to(DEV)
        self.cu_q, self.cu_k, self.ks, self.vs = (torch.from_numpy(x).to(DEV) for x in (c.cu_q, c.cu_k, c.k_scale, c.v_scale))


def arguments(c, d, out):
    """the argument list of fp8mi_attention_prefill as a dict, in order"""
    _T, Hq, DQK = c.q.shape
    kr = d.kr
    return dict(q=d.q.data_ptr(), q_dtype=CODE[d.q.dtype], T=d.T, Hq=Hq, DQK=DQK, DV=F.DV, ld_q=d.q.stride(0), k=d.k.data_ptr(), k_tok=d.k.stride(0), k_head=d.k.stride(1),
                k_rope=kr.data_ptr() if kr is not None else None, Hr=c.Hr, r_tok=kr.stride(0) if kr is not None else 0, r_head=kr.stride(1) if kr is not None else 0,
                v=d.v.data_ptr(), v_tok=d.v.stride(0), v_head=d.v.stride(1), Tk=d.Tk, Hkv=c.Hkv, k_scale=d.ks.data_ptr(), v_scale=d.vs.data_ptr(),
                scale_mode=L.KV_SCALE_HEAD if c.k_scale.size > 1 else L.KV_SCALE_TENSOR, B=len(c.q_lens), cu_q=d.cu_q.data_ptr(), cu_k=d.cu_k.data_ptr(),
                max_q_len=c.max_q_len, max_k_len=c.max_k_len, causal=int(c.causal), softmax_scale=c.softmax_scale, out=out.data_ptr(), out_dtype=CODE[out.dtype],
                ld_out=out.stride(0), stream=stream())


def run(lib, c, d=None, **change):
    """one fp8mi_attention_prefill of the case -> out (d.T, Hq, 128) on the CPU: rows the call did not write hold the sentinel"""
    d = Device(c) if d is None else d
    out = torch.full((d.T, c.q.shape[1] * F.DV), SENT_F, dtype=TORCH[c.out_dtype], device=DEV)
    with L.kernel_timer(4) as kt:
        L.check(lib.fp8mi_attention_prefill(*{**arguments(c, d, out), **change}.values()), "fp8mi_attention_prefill")
    torch.cuda.synchronize()
    assert len(kt.ms) == 1, "one launch"
    return out.reshape(d.T, c.q.shape[1], F.DV).cpu()


def within_tol(out, ref, vmax, what):
    got = out.double().numpy()
    assert not np.isnan(got).any(), what
    r = R.ratio(got, ref, vmax)
    print(f"{what}: max |out - ref| / max|V| = {r:.5f} (TOL_flash {F.TOL_flash})")
    assert r <= F.TOL_flash, (what, r)


@pytest.mark.parametrize("name", F.FLASH_CASES)
def test_within_tol_of_the_float64_reference(lib, name):
    c, e, ref, vmax = F.flash_case(name)
    out = run(lib, c)
    within_tol(out, ref, vmax, name)
    assert out.numel() > 0 and not out[torch.from_numpy(e.seq_lens == 0)].any(), "a row without a visible position is zero"


@pytest.mark.parametrize("causal", (False, True))
def test_nothing_at_or_beyond_k_len_is_read_and_unowned_rows_are_not_written(lib, causal):
    """k_lens 200 and 60, q_lens 40 and 3, G = 4 (W = 32): the next sequence's rows, 5 rows behind cu_k[B] and - under max_k_len = 150 - a
    sequence's own rows from 150 on are NaN patterns and junk; 3 rows of out are nobody's and tokens at or beyond max_q_len = 7 are not written.
    Causal: V NaN at position 195 (KV head 0, channel 9) leaves tile 0 (limits 161 .. 192) alone, makes tokens 35 .. 39 (limits above 195) NaN
    in that channel only, and tokens 32 .. 34 of tile 1 are the documented exception."""
    c = F.make_flash_case(45000, [200, 60], [40, 3], 8, 2, 192, causal=causal, Hr=2)
    d = Device(c, extra_k=5, extra_q=3)
    clean = run(lib, c, d)
    e = F.expand(c)
    within_tol(clean[:43], *F.reference(e), "clean")
    assert bool((clean[43:] == SENT_F).all()) and not bool((clean[:43] == SENT_F).any())
    short = run(lib, c, d, max_q_len=7)
    owned = torch.zeros(46, dtype=torch.bool)
    owned[:7], owned[40:43] = True, True
    assert torch.equal(bits(short[owned]), bits(clean[owned])) and bool((short[~owned] == SENT_F).all())
    clamped = run(lib, c, d, max_k_len=150)
    junk = torch.randint(0, 256, (d.Tk, 2, 128), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    junk.reshape(-1)[::7] = 0x7F
    junk = junk.to(DEV)
    for t in (d.k, d.v, d.kr):
        t[260:] = junk[260:, :, :t.shape[2]]   # behind cu_k[B]
    assert torch.equal(bits(run(lib, c, d)), bits(clean))
    for t in (d.k, d.v, d.kr):
        t[150:] = junk[150:, :, :t.shape[2]]   # sequence 0 from 150 on, and all of sequence 1
    assert torch.equal(bits(run(lib, c, d, max_k_len=150)[:40]), bits(clamped[:40]))
    if causal:
        d = Device(c)
        d.v[195, 0, 9] = 0x7F
        out = run(lib, c, d)
        same = torch.ones(out.shape[:2], dtype=torch.bool)
        same[32:40, :4] = False   # tile 1, the heads of KV head 0
        lanes = [ch for ch in range(128) if ch != 9]
        assert torch.equal(bits(out[same]), bits(clean[:43][same])) and bool(out[35:40, :4, 9].isnan().all())
        assert torch.equal(bits(out[35:40, :4][:, :, lanes]), bits(clean[35:40, :4][:, :, lanes]))


BAD = [(dict(T=-1), E_SHAPE), (dict(max_k_len=-1), E_SHAPE), (dict(DQK=64), E_SHAPE), (dict(DV=64), E_SHAPE), (dict(Hq=7), E_SHAPE), (dict(Hkv=0), E_SHAPE),
       (dict(k_rope=None), E_SHAPE), (dict(DQK=128), E_SHAPE), (dict(Hr=3), E_SHAPE), (dict(ld_q=8 * 192 - 1), E_SHAPE), (dict(ld_out=8 * 128 - 1), E_SHAPE),
       (dict(k_tok=112), E_SHAPE), (dict(v_head=-16), E_SHAPE), (dict(r_tok=48), E_SHAPE), (dict(q_dtype=9), E_ENUM), (dict(out_dtype=-1), E_ENUM),
       (dict(scale_mode=2), E_ENUM), (dict(causal=2), E_ENUM), (dict(Hq=34, ld_q=34 * 192, ld_out=34 * 128), E_UNSUPPORTED),
       (dict(softmax_scale=float("inf")), E_UNSUPPORTED), (dict(k_tok=264), E_UNSUPPORTED), (dict(r_head=72), E_UNSUPPORTED), (dict(T=1 << 29), E_UNSUPPORTED),
       (dict(max_k_len=1 << 31), E_UNSUPPORTED), (dict(q=None), E_NULL), (dict(v=None), E_NULL), (dict(cu_k=None), E_NULL), (dict(out=None), E_NULL),
       (dict(k="+8"), E_UNSUPPORTED), (dict(cu_q="+2"), E_UNSUPPORTED)]


@pytest.mark.parametrize("change,error", BAD, ids=[",".join(f"{k}={v}" for k, v in ch.items()) for ch, _ in BAD])
def test_bad_arguments_return_their_error_and_launch_nothing(lib, change, error):
    c = F.flash_case("q_len = k_len + 3")[0]   # DQK = 192, Hq = 8, Hkv = Hr = 2
    d = Device(c)
    out = torch.full((d.T, 8 * F.DV), SENT_F, device=DEV)
    args = arguments(c, d, out)
    change = {k: args[k] + int(v) if isinstance(v, str) else v for k, v in change.items()}   # "+n": the pointer moved by n bytes
    with L.kernel_timer(2) as kt:
        rc = lib.fp8mi_attention_prefill(*{**args, **change}.values())
    torch.cuda.synchronize()
    assert rc == error and len(kt.ms) == 0 and bool((out == SENT_F).all()), (rc, lib.fp8mi_last_error())


@pytest.mark.parametrize("per_head", (False, True))
def test_kv_quantize_bytes_and_sdpa_bits(N_, per_head):
    """the producer's bytes are the oracle's encode of x * (1 / scale), on a strided slice too; fp8_sdpa is fp8_attention on those bytes, bit for bit"""
    rng = np.random.default_rng(46000)
    x = rng.standard_normal((37, 3, 2, 128)).astype(np.float32)   # (T, H, k | v, D): the slices are strided
    scale = (np.abs(x[:, :, 0]).max(axis=(0, 2)) / 448.0 if per_head else np.array([np.abs(x).max() / 448.0])).astype(np.float32)
    xd = torch.from_numpy(x).to(DEV).to(torch.bfloat16)
    for rne, src in ((True, xd[:, :, 0]), (False, xd[:, :, 0]), (True, xd[:, :, 0].contiguous())):
        want = R.quantise(xd[:, :, 0].float().cpu().numpy(), scale.reshape(-1, 1) if per_head else scale, rne)
        assert np.array_equal(N_.fp8_attention_kv_quantize(src, torch.from_numpy(scale), L.ENC_RNE if rne else L.ENC_REFERENCE).cpu().numpy(), want)
    B, H, Hkv, S, Sk = 2, 4, 2, 45, 70
    q, k, v = (torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(DEV).to(torch.bfloat16) for s in ((B, H, S, 128), (B, Hkv, Sk, 128), (B, Hkv, Sk, 128)))
    ks, vs = (torch.tensor([0.01, 0.012], device=DEV), torch.tensor([0.011, 0.009], device=DEV)) if per_head else (None, None)
    rows = lambda t: t.transpose(1, 2).reshape(-1, t.shape[1], 128)   # noqa: E731
    dyn = lambda t: N_.fp8_amax(t) / 448.0                            # noqa: E731
    ks_, vs_ = (dyn(k), dyn(v)) if ks is None else (ks, vs)
    k8, v8 = N_.fp8_attention_kv_quantize(rows(k), ks_), N_.fp8_attention_kv_quantize(rows(v), vs_)
    cu = lambda n: torch.arange(0, (B + 1) * n, n, dtype=torch.int32, device=DEV)   # noqa: E731
    for causal in (False, True):
        want = N_.fp8_attention(rows(q), k8, v8, ks_, vs_, cu_seqlens_q=cu(S), cu_seqlens_k=cu(Sk), max_q_len=S, max_k_len=Sk, causal=causal)
        got = N_.fp8_sdpa(q, k, v, is_causal=causal, k_scale=ks, v_scale=vs)
        assert tuple(got.shape) == (B, H, S, 128) and torch.equal(bits(got.transpose(1, 2).reshape(-1, H, 128)), bits(want)) and not bool(got.isnan().any())


def test_graph_replay_on_new_lengths_and_contents(lib, N_):
    """captured on one batch, replayed several times after cu_seqlens_*, q, k, k_rope and v changed in place: the eager call's bits"""
    first = F.make_flash_case(47000, [33, 140], [3, 5], 4, 2, 192, causal=True)
    second = F.make_flash_case(47001, [150, 9], [6, 1], 4, 2, 192, causal=True)
    T, Tk = 8, 173

    def tensors(c):
        q, k, kr, v = np.zeros((T, 4, 192), np.float32), np.zeros((Tk, 2, 128), np.uint8), np.zeros((Tk, 1, 64), np.uint8), np.zeros((Tk, 2, 128), np.uint8)
        q[:c.q.shape[0]], k[:c.k.shape[0]], kr[:c.k.shape[0]], v[:c.k.shape[0]] = c.q, c.k, c.k_rope, c.v
        return [torch.from_numpy(x) for x in (q, k, kr, v, c.cu_q, c.cu_k, c.k_scale, c.v_scale)]

    q, k, kr, v, cu_q, cu_k, ks, vs = held = [x.to(DEV) for x in tensors(first)]
    call = lambda: N_.fp8_attention(q, k, v, ks, vs, k_rope=kr, cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, max_q_len=T, max_k_len=160, causal=True)   # noqa: E731
    call()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(out.cpu()), bits(call().cpu()))
    for dst, src in zip(held, tensors(second)):
        dst.copy_(src)
    eager = call().cpu()
    for _ in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(out.cpu()[:7]), bits(eager[:7]))
    within_tol(out.cpu()[:7], *F.reference(F.expand(second)), "graph replay")
