"""Scan the gfx950 code of a built library or object for DPP reads that follow a VALU write of their source register by
fewer than two wait states.  The assembler's hazard recogniser does not look inside inline-assembly blocks, so the DPP
reads of csrc/blsgpu_lin_absorb.h rely on a hand-placed s_nop and on the compiler leaving no register copy between the
blocks; this reads the disassembly and says whether that held.

    python tools/dpp_hazard_scan.py python-bls_amd/csrc/libblsgpu.so [more .so / .o files]

Prints one line per hazard and a count per file; exit status 1 if any was found."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def _tool(name):
    p = os.path.join(LLVM, name)
    return p if os.path.exists(p) else shutil.which(name)


def disassemble(path, workdir):
    """the device code of a host object or shared library, as llvm-objdump prints it"""
    fat, co = os.path.join(workdir, "fat.bin"), os.path.join(workdir, "dev.co")
    subprocess.check_call([shutil.which("objcopy") or _tool("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", path, fat])
    subprocess.check_call([_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + fat, "--output=" + co])
    return subprocess.run([_tool("llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout


def scan(text):
    """-> (number of DPP instructions, [(function, source register, wait states, the writing instruction)])"""
    ins, func, ndpp, bad = [], None, 0, []
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:", line)
        if m:
            func, ins = m.group(1), []
            continue
        m = re.match(r"^\s+(\S+)\s*(.*?)\s*//", line)
        if not m:
            continue
        op, args = m.group(1), m.group(2)
        if "_dpp" in op or "quad_perm" in args or "row_shr" in args or "row_shl" in args or "row_bcast" in args:
            ndpp += 1
            src = args.split(",")[1].strip().split(" ")[0]
            ws = 0
            for pop, pargs in reversed(ins[-4:]):
                if ws >= 2:
                    break
                if pop == "s_nop":
                    ws += int(pargs, 0) + 1
                    continue
                if pop.startswith("v_"):
                    dst = pargs.split(",")[0].strip()
                    regs = [dst]
                    mm = re.match(r"v\[(\d+):(\d+)\]", dst)
                    if mm:
                        regs = ["v%d" % i for i in range(int(mm.group(1)), int(mm.group(2)) + 1)]
                    if src in regs:
                        bad.append((func, src, ws, pop + " " + pargs))
                ws += 1
        ins.append((op, args))
    return ndpp, bad


def scan_file(path):
    with tempfile.TemporaryDirectory() as d:
        return scan(disassemble(path, d))


if __name__ == "__main__":
    total = 0
    for p in sys.argv[1:]:
        n, bad = scan_file(p)
        for func, src, ws, w in bad:
            print("%s: %s: a DPP read of %s comes %d wait state(s) after %s" % (p, func, src, ws, w))
        print("%s: %d DPP instructions, %d hazards" % (p, n, len(bad)))
        total += len(bad)
    sys.exit(1 if total else 0)
