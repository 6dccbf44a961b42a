"""The fused rotary embedding + cache appends (fp8mi_rope_kv_cache_append, fp8mi_mla_rope_cache_append) on the host, no GPU: the ABI's symbols
and constants, the argument checks through the built library (each runs before any HIP call), no scratch in the kernels, and the float32
definition of the rotation against float64."""
import os
import re
import subprocess
import sys

import pytest
import torch

import fp8_mi355x_lib as L
import rope_ref as R
from conftest import ROOT

E_NULL, E_SHAPE, E_ENUM, E_UNSUPPORTED = -1, -2, -3, -4   # include/fp8mi.h
P = 0x100000   # a 16-byte aligned fake device pointer: the calls below must fail before anything dereferences it


@pytest.fixture(scope="module")
def lib():
    return L.load()


def test_symbols_bindings_constants_and_ops(lib):
    header = open(os.path.join(ROOT, "include", "fp8mi.h")).read()
    for name, n in (("fp8mi_rope_kv_cache_append", 37), ("fp8mi_mla_rope_cache_append", 28)):
        assert re.search(r"\bint %s\(" % name, header) and len(L.SIGNATURES[name][1]) == n and getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    assert (L.ROPE_NEOX, L.ROPE_GPTJ) == (0, 1) and "#define FP8MI_ROPE_NEOX 0" in header and "#define FP8MI_ROPE_GPTJ 1" in header
    assert lib.fp8mi_version() == 0x000400
    import fp8_mi355x_native as N
    assert callable(N.fp8_rope_kv_cache_append) and callable(N.fp8_mla_rope_cache_append)


def rope(lib, q=P, k=P, v=P, dtype=L.BF16, T=4, Hq=4, Hkv=2, D=128, ld=None, pos=P, pos_bytes=8, cs=P, cs_dtype=L.F32, max_pos=64, ld_cs=None, rot_dim=128,
         style=L.ROPE_NEOX, qw=None, kw=None, q_out=P, kc=P, vc=P, nb=4, bs=16, slots=P, slot_bytes=8, ks=P, vs=P, scale_mode=0, enc=L.ENC_RNE, k8=None, v8=None):
    ld_q, ld_kv = (Hq * D, Hkv * D) if ld is None else (ld, ld)
    return lib.fp8mi_rope_kv_cache_append(q, k, v, dtype, T, Hq, Hkv, D, ld_q, ld_kv, ld_kv, pos, pos_bytes, cs, cs_dtype, max_pos, rot_dim if ld_cs is None else ld_cs,
                                          rot_dim, style, qw, kw, 1e-6, q_out, ld_q, kc, vc, nb, bs, slots, slot_bytes, ks, vs, scale_mode, enc, k8, v8, None)


def mla(lib, kv_c=P, k_pe=P, q_pe=P, dtype=L.BF16, T=4, Hq=8, ld_c=512, pos=P, pos_bytes=4, cs=P, cs_dtype=L.BF16, max_pos=64, ld_cs=64, style=L.ROPE_GPTJ, kvw=None,
        q_out=P, cache=P, nb=4, bs=16, slots=P, slot_bytes=4, kvs=P, enc=L.ENC_RNE):
    return lib.fp8mi_mla_rope_cache_append(kv_c, k_pe, q_pe, dtype, T, Hq, ld_c, 64, Hq * 64, pos, pos_bytes, cs, cs_dtype, max_pos, ld_cs, style, kvw, 1e-6, q_out,
                                           Hq * 64, cache, nb, bs, slots, slot_bytes, kvs, enc, None)


def test_argument_errors_without_gpu(lib):
    err = lambda: lib.fp8mi_last_error()   # noqa: E731
    assert rope(lib, T=-1) == E_SHAPE and rope(lib, Hq=-1) == E_SHAPE and rope(lib, Hkv=0) == E_SHAPE and rope(lib, D=96) == E_SHAPE and rope(lib, bs=24) == E_SHAPE
    assert rope(lib, rot_dim=4) == E_SHAPE and b"rot_dim" in err() and rope(lib, rot_dim=20) == E_SHAPE and rope(lib, rot_dim=136) == E_SHAPE
    assert rope(lib, ld=255) == E_SHAPE and b"leading dimension" in err() and rope(lib, ld_cs=120) == E_SHAPE and rope(lib, max_pos=0) == E_SHAPE and b"max_pos" in err()
    assert rope(lib, dtype=3) == E_ENUM and rope(lib, cs_dtype=7) == E_ENUM and rope(lib, style=2) == E_ENUM and b"rope_style" in err()
    assert rope(lib, scale_mode=2) == E_ENUM and rope(lib, enc=2) == E_ENUM and rope(lib, slot_bytes=2) == E_ENUM and rope(lib, pos_bytes=16) == E_ENUM and b"pos_bytes" in err()
    assert rope(lib, k=None) == E_NULL and b"fp8mi_rope_kv_cache_append: NULL" in err() and rope(lib, q_out=None) == E_NULL and rope(lib, pos=None) == E_NULL
    assert rope(lib, kc=None) == E_NULL and rope(lib, slots=None) == E_NULL   # the caches and slot_mapping: all three or none
    assert rope(lib, q=P + 1) == E_UNSUPPORTED and b"aligned" in err() and rope(lib, k8=P + 8) == E_UNSUPPORTED and rope(lib, qw=P + 4) == E_UNSUPPORTED
    assert rope(lib, pos=P + 4) == E_UNSUPPORTED and rope(lib, pos=P + 4, pos_bytes=4, q=None) == E_NULL
    none = dict(q=None, k=None, v=None, pos=None, cs=None, q_out=None, kc=None, vc=None, slots=None, ks=None, vs=None)
    assert rope(lib, T=0, **none) == 0 and rope(lib, T=0, rot_dim=12, **none) == E_SHAPE   # a no-op that still validates
    assert mla(lib, ld_c=511) == E_SHAPE and mla(lib, max_pos=0) == E_SHAPE and mla(lib, ld_cs=63) == E_SHAPE and mla(lib, bs=8) == E_SHAPE and mla(lib, Hq=-1) == E_SHAPE
    assert mla(lib, style=5) == E_ENUM and mla(lib, dtype=9) == E_ENUM and mla(lib, pos_bytes=2) == E_ENUM and mla(lib, enc=3) == E_ENUM
    assert mla(lib, Hq=129) == E_UNSUPPORTED and b"MLA_MAX_HEADS" in err() and mla(lib, cache=P + 4) == E_UNSUPPORTED and mla(lib, kvw=P + 8) == E_UNSUPPORTED
    assert mla(lib, cache=None) == E_NULL and b"fp8mi_mla_rope_cache_append: NULL" in err() and mla(lib, q_pe=None) == E_NULL and mla(lib, kvs=None) == E_NULL
    assert mla(lib, T=0, kv_c=None, k_pe=None, q_pe=None, pos=None, cs=None, q_out=None, cache=None, slots=None, kvs=None) == 0


def test_the_kernels_use_no_scratch():
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "check_spills.py"), "fp8mi_rope.hip"], stdout=subprocess.DEVNULL)


@pytest.mark.parametrize("style", ("neox", "gptj"))
@pytest.mark.parametrize("rot_dim", (8, 24, 64))
def test_rotate32_is_within_three_roundings_of_rotate64(rot_dim, style):
    gen = torch.Generator().manual_seed(rot_dim)
    x = (torch.randn((9, 3, 64), generator=gen) * 4).to(torch.bfloat16)
    ang = torch.rand((17, rot_dim // 2), generator=gen) * 6.3
    table, pos = torch.cat([ang.cos(), ang.sin()], dim=1), torch.randint(0, 17, (9,), generator=gen)
    y32, (y64, mag) = R.rotate32(x, table, pos, rot_dim, style), R.rotate64(x, table, pos, rot_dim, style)
    assert bool((torch.from_numpy(y64) - y32.double()).abs().le(2.0 ** -22 * torch.from_numpy(mag)).all())
    assert torch.equal(y32[..., rot_dim:], x.float()[..., rot_dim:]) and not torch.equal(y32[..., :rot_dim], x.float()[..., :rot_dim])
