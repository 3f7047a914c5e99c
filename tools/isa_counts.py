"""Static instruction-class counts per kernel of one csrc/*.hip file, from its gfx950 assembly.

Compiles the file (device side only) with the Makefile's compiler and flags and prints, for every kernel in it:
branches (s_branch + s_cbranch_*), other SALU (s_* without waits, nops, barriers, program end, priority / sleep hints
and scalar memory loads), VALU (v_* without MFMAs), MFMAs (v_mfma_*, compiler-issued or inline asm) and the scratch
bytes per lane (.amdhsa_private_segment_fixed_size).  The counts are static and cover the whole kernel, every path
once; they say how much code an epilogue or an address computation is, not how often it runs.

usage: python tools/isa_counts.py climate-super-resolution_amd/csrc/conv_wr.hip [name-filter ...] [--asm OUT.s]
       python tools/isa_counts.py OUT.s [name-filter ...]        (counts a kept assembly file)
"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "climate-super-resolution_amd", "csrc")
NOT_SALU = ("s_waitcnt", "s_nop", "s_barrier", "s_endpgm", "s_setprio", "s_sleep", "s_load_", "s_buffer_load_", "s_code_end",
            "s_inst_prefetch", "s_sethalt", "s_trap")


def make_flags(src):
    """(compiler, flags) the Makefile builds `src` with: HIPCC, CXXFLAGS with $(ARCH), plus the file's own `+=`."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    var = {}
    for m in re.finditer(r"^(\w+)\s*\?=\s*(.*)$", text, re.M):
        var[m.group(1)] = m.group(2).strip()
    obj = os.path.splitext(os.path.basename(src))[0] + ".o"
    extra = " ".join(m.group(1) for m in re.finditer(r"^%s:\s*CXXFLAGS\s*\+=\s*(.*)$" % re.escape(obj), text, re.M))
    flags = (var["CXXFLAGS"] + " " + extra).replace("$(ARCH)", os.environ.get("ARCH", var["ARCH"]))
    return os.environ.get("HIPCC", var["HIPCC"]), flags.split()


def assemble(src):
    hipcc, flags = make_flags(src)
    cmd = [hipcc] + flags + ["--cuda-device-only", "-S", "-o", "-", os.path.abspath(src)]
    return subprocess.run(cmd, cwd=CSRC, check=True, capture_output=True, text=True).stdout


def demangle(names):
    for tool in ("c++filt", "llvm-cxxfilt"):
        try:
            out = subprocess.run([tool] + names, check=True, capture_output=True, text=True).stdout.split("\n")
            return dict(zip(names, out))
        except (OSError, subprocess.CalledProcessError):
            pass
    return {n: n for n in names}  # no demangler: the mangled symbols


def count(asm):
    """-> {kernel symbol: dict(branch, salu, valu, mfma, scratch)} for the .amdhsa_kernel symbols of `asm`."""
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    res, cur, desc = {}, None, None
    for raw in asm.split("\n"):
        s = raw.split(";")[0].strip()
        if not s:
            continue
        m = re.fullmatch(r"(\S+):", s)
        if m:  # a kernel's symbol opens it; its .Lfunc_end or any other function's symbol closes it; block labels do not
            if m.group(1) in kernels:
                cur = res.setdefault(m.group(1), dict(branch=0, salu=0, valu=0, mfma=0, scratch=0))
            elif s.startswith(".Lfunc_end") or not s.startswith("."):
                cur = None
            continue
        if s.startswith("."):
            m = re.match(r"\.amdhsa_kernel\s+(\S+)", s)
            if m:
                desc = m.group(1)
            m = re.match(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", s)
            if m and desc in res:
                res[desc]["scratch"] = int(m.group(1))
            continue
        if cur is None:
            continue
        op = s.split()[0]
        if op == "s_branch" or op.startswith("s_cbranch"):
            cur["branch"] += 1
        elif op.startswith("s_"):
            cur["salu"] += not op.startswith(NOT_SALU)
        elif op.startswith("v_mfma") or op.startswith("v_smfma"):
            cur["mfma"] += 1
        elif op.startswith("v_"):
            cur["valu"] += 1
    return res


def main():
    args = sys.argv[1:]
    out = None
    if "--asm" in args:
        i = args.index("--asm")
        out = args[i + 1]
        del args[i:i + 2]
    if not args:
        print(__doc__)
        return 2
    asm = open(args[0]).read() if args[0].endswith(".s") else assemble(args[0])  # (a kept --asm file: counted as is)
    if out:
        open(out, "w").write(asm)
    res = count(asm)
    names = demangle(sorted(res))
    print(f"{'kernel':<72} {'branch':>6} {'SALU':>6} {'VALU':>6} {'MFMA':>5} {'scratch':>7}")
    for sym, nice in sorted(names.items(), key=lambda kv: kv[1]):
        nice = re.sub(r"^void |\(anonymous namespace\)::|\(.*\)$", "", nice)
        if args[1:] and not any(f in nice for f in args[1:]):
            continue
        c = res[sym]
        print(f"{nice:<72} {c['branch']:>6} {c['salu']:>6} {c['valu']:>6} {c['mfma']:>5} {c['scratch']:>7}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
