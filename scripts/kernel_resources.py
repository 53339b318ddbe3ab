#!/usr/bin/env python
"""VGPRs / SGPRs / scratch / LDS / occupancy of the kernels in a build directory's gfx950 objects (the metadata note of each code object).

    python scripts/kernel_resources.py [build-dir] [name-substring ...]
"""
import glob
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def notes(obj, tool_args=("--notes",)):
    with tempfile.TemporaryDirectory() as td:
        co = os.path.join(td, "co")
        r = subprocess.run([LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                            "--input=" + obj, "--output=" + co], capture_output=True)
        if r.returncode or not os.path.exists(co) or os.path.getsize(co) == 0:
            # a host object with an embedded fat binary: pull the section out first
            fb = os.path.join(td, "fb")
            subprocess.run([LLVM + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fb, obj], capture_output=True)
            if not os.path.exists(fb):
                return ""
            subprocess.run([LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                            "--input=" + fb, "--output=" + co], capture_output=True)
        if not os.path.exists(co):
            return ""
        return subprocess.run([LLVM + "/llvm-readelf"] + list(tool_args) + [co], capture_output=True, text=True).stdout


def kernels(obj):
    """{demangled kernel name (without its argument list): {metadata key: value}} of an object's gfx950 code object."""
    out = {}
    for blk in re.split(r"\n\s+- \.agpr_count", notes(obj))[1:]:
        g = lambda k: (re.search(r"\.%s:\s+(\S+)" % k, blk) or [None, "?"])[1]
        dem = subprocess.run(["c++filt", g("name")], capture_output=True, text=True).stdout.strip()
        out[re.sub(r"\(.*", "", dem)] = {k: g(k) for k in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
                                                          "group_segment_fixed_size")}
    return out


def function_sizes(obj):
    """{mangled name: bytes of code} of every function symbol (kernels and out-of-line device functions) in an object's gfx950 code object:
    the symbol table is the only place a device function that is no kernel shows up (the metadata note lists kernels, with their callees'
    scratch and registers folded in)."""
    out = {}
    for l in notes(obj, ("--symbols", "--wide")).splitlines():
        p = l.split()
        if len(p) >= 8 and p[3] == "FUNC" and p[6] != "UND":
            out[p[7]] = int(p[2], 0) if not p[2].isdigit() else int(p[2])
    return out


def listing(src, out, flags=("-O3",)):
    """The gfx950 assembly listing of one translation unit, compiled with the flags of __graft_entry__.build_library (device side only)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off", "-fPIC"] + os.environ.get("SNAPGPU_BUILD_FLAGS", "").split() + list(flags)
    r = subprocess.run(cmd + ["--cuda-device-only", "-S", src, "-o", out], capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError(r.stderr[-2000:])
    return out


def function_info(path):
    """{mangled name: {codeLenInByte, ScratchSize, NumVgprs, TotalNumSgprs}} of every function of a listing -- kernels AND out-of-line device
    functions -- from the `; Function info:` block the compiler writes after each: a function's OWN figures (a kernel's metadata folds its
    callees' in).  Resource figures only; no instruction is looked at.  (How many SGPRs a function parks in VGPR lanes is not among them: the
    compiler states that count for kernels only.  SGPRs that find no free VGPR lane go to scratch and show up in ScratchSize.)"""
    out, name = {}, None
    for l in open(path, errors="replace"):
        m = re.match(r"\s*\.type\s+(\S+),@function", l)
        if m:
            name = m.group(1)
            continue
        m = re.match(r"; (codeLenInByte|ScratchSize|NumVgprs|TotalNumSgprs)\s*[=:]\s*(\d+)", l)
        if m and name:
            out.setdefault(name, {})[m.group(1)] = int(m.group(2))
    return out


def main():
    bdir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "snap_amd", "build")
    pats = sys.argv[2:]
    for obj in sorted(glob.glob(os.path.join(bdir, "*.o"))):
        for dem, m in kernels(obj).items():
            if pats and not any(p in dem for p in pats):
                continue
            print("%-22s %-70s vgpr %3s sgpr %3s spill(v/s) %s/%s scratch %5s B/lane lds %6s" % (
                os.path.basename(obj), dem[:70], m["vgpr_count"], m["sgpr_count"], m["vgpr_spill_count"], m["sgpr_spill_count"],
                m["private_segment_fixed_size"], m["group_segment_fixed_size"]))
        for name, size in sorted(function_sizes(obj).items()):
            dem = re.sub(r"\(.*", "", subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip())
            if "_fn" in name and (not pats or any(p in dem for p in pats)):
                print("%-22s %-70s function, %6d bytes of code" % (os.path.basename(obj), dem[:70], size))


if __name__ == "__main__":
    main()
