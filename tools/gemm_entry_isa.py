#!/usr/bin/env python3
"""What the ring-tile GEMM kernels do between kernel entry and their first stage DMA, read from the gfx950 ISA (no GPU needed; the
cross-compile of csrc/fp8mi_gemm.hip takes minutes).  Per kernel instance of the product library:

  head    instructions from the kernel's first to its first `buffer_load_dwordx4 ... lds`, the s_waitcnt among them, and whether one of
          those is a full `vmcnt(0)`
  flat    flat_* instructions in the whole kernel (C, bias and row scales are generic pointers: their accesses are flat and stay), and of
          those the volatile ones: `flat_load_dword ... sc0 sc1` (ld-v: a word of LDS read through a generic pointer - none may be left)
          and `flat_store_dword ... sc0 sc1` (st-v: the same for a write; the system-scope reset of the split-K arrival counter is
          one too and stays)
  s_load  single-dword scalar loads (the epilogue's per-tensor scalars; kernel arguments load as x2 .. x16)
  regs    VGPRs + AGPRs, LDS bytes, scratch bytes

    python tools/gemm_entry_isa.py [--tree PACKAGE_DIR] [--label NAME] [--all] [--asm FILE.s]
PACKAGE_DIR defaults to this tree's fp8-mps-metal_amd (give a checkout of another commit to compare); --all lists every instance
instead of the e4m3 tensorwise ones and one line of totals per other family."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CXXFILT = os.environ.get("CXXFILT") or shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "c++filt"
FAMILIES = ("gemm_kernel<", "gemm_fmt_kernel<", "gemm_mxfp8_kernel<", "gemm_mxfp4_kernel<", "gemm_mxw4a8_kernel<", "gemm_blockwise_kernel<", "gemm_grouped_kernel<")


def compile_asm(pkg):
    subprocess.check_call(["make", "-s", "-C", pkg, "csrc/fp8mi_gemm256_loop_fmt.inc"])
    out = os.path.join(tempfile.mkdtemp(prefix="gemm_entry_isa_"), "fp8mi_gemm.s")
    subprocess.check_call([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-fno-gpu-rdc", "--offload-device-only", "-S",
                           os.path.join(pkg, "csrc", "fp8mi_gemm.hip"), "-o", out])
    return out


def kernels(asm_path):
    """-> [(mangled name, [instruction lines], {metadata})] of every kernel function in the file"""
    text = open(asm_path).read().splitlines()
    out, name, body = [], None, None
    for line in text:
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        s = line.strip()
        if s.startswith(".amdhsa_kernel") or s.startswith(".section") or s.startswith(".text"):
            continue
        m = re.match(r"^; (NumVgprs|NumAgprs|TotalNumVgprs|ScratchSize|LDSByteSize|Occupancy): (\d+)", s)
        if m:
            out_meta = out[-1][2] if out and out[-1][0] == name else None
            if out_meta is None:
                out.append((name, body, {}))
                out_meta = out[-1][2]
            out_meta[m.group(1)] = int(m.group(2))
            continue
        if s and not s.startswith((";", ".", "//")) and not s.endswith(":"):
            body.append(s.split(";")[0].strip())
    return out


def report(name, body, meta):
    first = next((i for i, s in enumerate(body) if s.startswith("buffer_load_dwordx4") and " lds" in s), None)
    head = body[:first] if first is not None else []
    waits = [s for s in head if s.startswith("s_waitcnt")]
    full = sum(1 for s in waits if re.search(r"vmcnt\(0\)", s))
    flat = sum(1 for s in body if s.startswith("flat_"))
    ldv = sum(1 for s in body if s.startswith("flat_load_dword ") and "sc0 sc1" in s)
    stv = sum(1 for s in body if s.startswith("flat_store_dword ") and "sc0 sc1" in s)
    sload = sum(1 for s in body if s.startswith("s_load_dword "))
    return dict(name=name, head=len(head) if first is not None else -1, waits=len(waits), full=full, flat=flat, ldv=ldv, stv=stv, sload=sload,
                regs=meta.get("TotalNumVgprs", meta.get("NumVgprs", -1)), vgpr=meta.get("NumVgprs", -1), lds=meta.get("LDSByteSize", -1),
                scratch=meta.get("ScratchSize", -1), occ=meta.get("Occupancy", -1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.join(ROOT, "fp8-mps-metal_amd"))
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--asm", default=None, help="read this assembly file instead of compiling")
    a = ap.parse_args()
    ks = kernels(a.asm or compile_asm(a.tree))
    names = subprocess.run([CXXFILT], input="\n".join(k[0] for k in ks), capture_output=True, text=True, check=True).stdout.splitlines()
    rows = []
    for (mangled, body, meta), dem in zip(ks, names):
        dem = re.sub(r"^void \(anonymous namespace\)::", "", dem).split("(")[0]
        if dem.startswith(FAMILIES):
            rows.append(report(dem, body, meta))
    print(f"# {a.label}: ring-tile instances of csrc/fp8mi_gemm.hip, gfx950, -O3 ({len(rows)} kernels)")
    print(f"{'kernel':62s} {'head':>5s} {'waits':>5s} {'vmcnt(0)':>8s} {'flat':>5s} {'ld-v':>4s} {'st-v':>4s} {'s_load':>6s} {'VGPR':>5s} {'V+A':>5s} {'LDS':>7s} {'scratch':>7s}")
    fmt = lambda r: f"{r['name'][:62]:62s} {r['head']:5d} {r['waits']:5d} {r['full']:8d} {r['flat']:5d} {r['ldv']:4d} {r['stv']:4d} {r['sload']:6d} {r['vgpr']:5d} {r['regs']:5d} {r['lds']:7d} {r['scratch']:7d}"  # noqa: E731
    for r in rows:
        if a.all or r["name"].startswith("gemm_kernel<"):
            print(fmt(r))
    for fam in FAMILIES[1:]:
        mine = [r for r in rows if r["name"].startswith(fam)]
        if mine:
            print(f"{fam[:-1] + ' x ' + str(len(mine)):62s} head {min(r['head'] for r in mine)}..{max(r['head'] for r in mine)}, vmcnt(0) in head {sum(r['full'] for r in mine)}, "
                  f"flat ld-v {sum(r['ldv'] for r in mine)} st-v {sum(r['stv'] for r in mine)}, s_load {min(r['sload'] for r in mine)}..{max(r['sload'] for r in mine)}, scratch {max(r['scratch'] for r in mine)}")
    bad = [r["name"] for r in rows if r["ldv"] or r["full"] or r["scratch"]]
    print(f"# kernels with a volatile flat load, a vmcnt(0) ahead of the first stage, or scratch: {len(bad)} of {len(rows)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
