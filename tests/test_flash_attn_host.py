"""fp8mi_attention_prefill on the host, no GPU: E_flash recomputed and pinned; the symbols and their argument lists; the geometry helpers of
csrc/fp8mi_attn.h against the Python mirror."""
import os
import re

import fp8_mi355x_lib as L
import flash_attn_ref as F
import paged_attn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_model_stays_within_E_flash():
    worst = F.measure_E_flash()
    assert F.E_flash - 1e-5 <= worst <= F.E_flash and F.TOL_flash == 2 * F.E_flash and F.E_flash < 2.0 ** -4, worst
    assert len(F.FLASH_CASES) == 12 + 12 + 2 + 1 + 2 + 3 + 1 + 1 + 1 and R.WAVES == 4
    assert all(c.q.shape[0] > 0 and (vmax > 0).any() for c, _e, _ref, vmax in map(F.flash_case, F.FLASH_CASES))


def test_symbols_constants_and_geometry_match_the_sources():
    lib, hdr = L.load(), open(os.path.join(ROOT, "include", "fp8mi.h")).read()
    for name, n in (("fp8mi_attn_kv_quantize", 12), ("fp8mi_attention_prefill", 33)):
        assert re.search(r"\bint " + name + r"\s*\(", hdr)
        assert len(L.SIGNATURES[name][1]) == n and getattr(lib, name).argtypes == L.SIGNATURES[name][1]
    shared = open(os.path.join(ROOT, "fp8-mps-metal_amd", "csrc", "fp8mi_attn.h")).read()
    const = lambda name: int(re.search(r"constexpr int " + name + r" = (\d+);", shared).group(1))   # noqa: E731
    assert const("kAttnFlashCols") == F.COLS == L.ATTN_FLASH_COLS and const("kAttnFlashDV") == F.DV == L.ATTN_FLASH_DV
    assert const("kAttnFlashRope") == F.ROPE == L.ATTN_FLASH_ROPE and const("kAttnFlashWaves") == 4
    assert "kAttnFlashCols / kAttnMaxGroup * fp8mi_attn_tile_tokens(Hq, Hkv)" in shared   # W, the mirror of which is:
    assert [F.tokens_per_workgroup(g, 1) for g in (1, 4, 5, 16)] == [128, 32, 24, 8] and F.q_tiles(65, 8, 2) == 3 and F.q_tiles(64, 8, 2) == 2
