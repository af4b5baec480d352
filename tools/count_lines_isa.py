#!/usr/bin/env python3
"""Count the instructions of k_ml_lines2 / k_ml_lines4 per basic block, by opcode class and by the source function they
were expanded from (profiles/r08_lines2_resources.txt).  Input: the ISA of translation unit 3 with line tables,

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -DBLSGPU_TU=3 --cuda-device-only -S -gline-tables-only \
          -o tu3.s python-bls_amd/csrc/blsgpu_api.hip
    python3 tools/count_lines_isa.py tu3.s [--csrc DIR] [kernel ...]

(--csrc: the directory of the sources the ISA was compiled from, when it is not this tree's -- the "before" half of a table.)

A document's tool, not a test: it reads text and prints a table.  The tangent loop is the largest block of a kernel that
branches back to itself; the chord blocks are the straight-line code between two entries of it.
"""
import collections
import os
import re
import sys

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "python-bls_amd", "csrc")
ATTR = re.compile(r"__attribute__\(\([^)]*(\([^)]*\))?[^)]*\)\)|__launch_bounds__\([^)]*\)")
DEF = re.compile(r"__(?:device|global)__[^;(]*?\b([A-Za-z_]\w*)\s*\(")


def source_functions(path):
    """line number -> name of the function whose definition precedes it (good enough for headers of small helpers)"""
    out, cur = {}, "?"
    try:
        with open(path) as f:
            for n, line in enumerate(f, 1):
                m = DEF.search(ATTR.sub("", line))
                if m and not line.lstrip().startswith("//"):
                    cur = m.group(1)
                out[n] = cur
    except OSError:
        pass
    return out


def opclass(op, text):
    if op == "v_mad_i64_i32":
        return "mad"
    if "quad_perm" in text or "row_" in text or op.endswith("_dpp"):
        return "dpp"
    if op.startswith("v_cndmask"):
        return "select"
    if op.startswith(("v_add", "v_sub", "v_lshl_add", "v_add3", "v_lshl_or")):
        return "add/sub"
    if op.startswith(("v_and", "v_or", "v_xor", "v_bfe", "v_bfi")):
        return "mask"
    if op.startswith(("v_ashr", "v_lshr", "v_lshl", "v_alignbit")):
        return "shift"
    if op.startswith("v_mul"):
        return "mul"
    if op.startswith(("v_mov", "v_accvgpr", "v_readfirstlane")):
        return "mov"
    if op.startswith("v_cmp"):
        return "cmp"
    if op.startswith("v_"):
        return "valu-other"
    if op.startswith("global_store"):
        return "gstore"
    if op.startswith("global_") or op.startswith("flat_"):
        return "gload"
    if op.startswith("scratch_") or op.startswith("buffer_"):
        return "scratch"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("s_waitcnt"):
        return "waitcnt"
    if op.startswith("s_"):
        return "salu"
    return "other"


def blocks_of(lines, kernel):
    """[(label, [(op, text, file, line)])] of one function"""
    files, funcs = {}, {}
    start = None
    for i, l in enumerate(lines):
        m = re.match(r'\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', l)
        if m:
            files[int(m.group(1))] = os.path.basename(m.group(3) or m.group(2))
        if start is None and re.match(r"^_ZN\w*%s\w*:" % kernel, l):
            start = i
    if start is None:
        raise SystemExit("kernel %s not found" % kernel)
    out, cur, loc = [], ("entry", []), ("?", 0)
    for l in lines[start + 1:]:
        s = l.strip()
        if s.startswith(".Lfunc_end"):
            break
        m = re.match(r"\.loc\s+(\d+)\s+(\d+)", s)
        if m:
            loc = (files.get(int(m.group(1)), "?"), int(m.group(2)))
            continue
        m = re.match(r"(\.LBB\d+_\d+):", s)
        if m:
            out.append(cur)
            cur = (m.group(1), [])
            continue
        if not s or s.startswith((".", ";", "//")) or s.endswith(":"):
            continue
        op = s.split()[0]
        cur[1].append((op, s, loc[0], loc[1]))
    out.append(cur)
    return out


def source_of(fn, line, maps):
    if fn not in maps:
        maps[fn] = source_functions(os.path.join(CSRC, fn))
    name = maps[fn].get(line, "?")
    if fn.startswith("fp28_mul"):
        return "fp28_dot* (product + reduction)"
    return "%s" % name


def report(path, kernel):
    with open(path) as f:
        lines = f.read().split("\n")
    blocks = blocks_of(lines, kernel)
    maps = {}
    print("== %s" % kernel)
    big = [(lab, ins) for lab, ins in blocks if len(ins) >= 1000]
    for lab, ins in big:
        loop = any(i[0].startswith("s_cbranch") and lab in i[1] for i in ins)
        n = len(ins)
        mad = sum(1 for i in ins if i[0] == "v_mad_i64_i32")
        valu = sum(1 for i in ins if i[0].startswith("v_"))
        print("-- block %s (%s): %d instructions, %d VALU, %d v_mad_i64_i32, %d VALU that are not" %
              (lab, "loop on itself" if loop else "straight line", n, valu, mad, valu - mad))
        by = collections.defaultdict(collections.Counter)
        for op, text, fn, line in ins:
            c = opclass(op, text)
            if c == "mad":
                continue
            by[source_of(fn, line, maps)][c] += 1
        cols = sorted({c for v in by.values() for c in v})
        print("   %-34s %6s  %s" % ("source (non-mad instructions)", "total", " ".join("%9s" % c for c in cols)))
        for src, cnt in sorted(by.items(), key=lambda kv: -sum(kv[1].values())):
            print("   %-34s %6d  %s" % (src, sum(cnt.values()), " ".join("%9s" % (cnt[c] or "") for c in cols)))
        tot = collections.Counter()
        for cnt in by.values():
            tot.update(cnt)
        print("   %-34s %6d  %s" % ("all", sum(tot.values()), " ".join("%9d" % tot[c] for c in cols)))


if __name__ == "__main__":
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    rest = sys.argv[2:]
    if rest[:1] == ["--csrc"]:
        CSRC = rest[1]
        rest = rest[2:]
    for k in (rest or ["k_ml_lines2", "k_ml_lines4"]):
        report(sys.argv[1], k)
