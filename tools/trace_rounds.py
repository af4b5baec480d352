"""Diagnostic: run the first n rounds of any program of vmgen.emit.build_tables() on the GPU from a seeded scratchpad image, through
the test-only library csrc/libblsgpu_vmcheck.so (the ordinary build: no stamps library needed), and compare every slot with
vmgen/tablesim.py, bisecting to the first round whose result differs and printing that round's lane records.
    python3 tools/trace_rounds.py            lists the programs
    python3 tools/trace_rounds.py mscript    (or mpscript, mp2, fscript, slow, h2, or a directly called segment such as d1_a, g2_add)
tests/test_gpu_vm.py asserts the same comparison at every segment boundary."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "python-bls_amd"), os.path.join(ROOT, "tests")]
import checklib                                           # noqa: E402
import vm_vectors as V                                    # noqa: E402
from vmgen import emit                                    # noqa: E402

progs, data, consts = V.production()
by_name = {name: (op, rounds) for name, op, rounds, cuts in progs}
if len(sys.argv) < 2 or sys.argv[1] not in by_name:
    print("programs:", " ".join(by_name))
    sys.exit(0 if len(sys.argv) < 2 else 2)
prog = sys.argv[1]
op, rounds = by_name[prog]
img = V.production_image(prog, op, rounds, data, consts)
nslots = len(img)
lib = checklib.load("libblsgpu_vmcheck", "blsgpu_vm_check")
t16 = np.array(list(data) + [0] * (len(data) & 1), dtype=np.uint32)
table = t16[0::2] | (t16[1::2] << 16)
image = np.frombuffer(b"".join(v.to_bytes(48, "little") for v in img), dtype=np.uint32)


def gpu(n):
    if n == 0:
        return [v % V.Q for v in img]
    hdr = np.array([n, nslots, len(data), 0, 0, 1, 0, 0] + [x for r in rounds[:n] for x in r], dtype=np.uint32)
    w, out = np.concatenate([hdr, table, image]), np.zeros(nslots * 12 + V.TRAILER, dtype=np.uint32)
    rc = lib(V.OPS[op], w.ctypes.data, w.size, 1, out.ctypes.data, out.size)
    assert rc == 0, "blsgpu_vm_check returned %d" % rc
    b = out.tobytes()
    return [int.from_bytes(b[48 * s:48 * s + 48], "little") % V.Q for s in range(nslots)]


def cpu(n):
    return V.tablesim_run(data, img, rounds[:n], op in V.LIGHT_OPS)[0]


def same(n):
    return gpu(n) == cpu(n)


print("program", prog, "under", op, "rounds", len(rounds), "slots", nslots, "full run matches:", same(len(rounds)))
lo, hi = 0, len(rounds)
if not same(hi):
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if same(mid):
            lo = mid
        else:
            hi = mid
    off, meta = rounds[hi - 1]
    a, b = gpu(hi), cpu(hi)
    bad = [s for s in range(nslots) if a[s] != b[s]]
    print("first differing round: #%d kind %d K %d levels %d MN %d; slots %s" % (hi - 1, meta & 3, (meta >> 8) & 255, (meta >> 16) & 3, (meta >> 18) & 255, bad[:12]))
    rl = emit.kpad((meta >> 8) & 255) if meta & 3 == 1 else 4
    for lane in range(64):
        rec = data[off + rl * lane: off + rl * (lane + 1)]
        if rec[0] != 0xFFFF and (rec[0] // 3 in bad if meta & 3 == 1 else rec[2] // 3 in bad):
            print("  lane", lane, "record", rec)
