"""CPU: the decision the VM check library makes before it launches (csrc/vm_check_plan.h verify(): which programs run_rounds may be
given), compiled with g++ into a stand-alone program and run on the cases of tests/vm_refusals.py and on every program
tests/test_gpu_vm.py uploads -- all of which it must accept.  Needs no GPU."""
import os
import struct
import subprocess

import vm_refusals as RF
import vm_vectors as V

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "python-bls_amd", "csrc")

# input: per case {light, teams, output words, input words, the words}; output: one return code per line
DRIVER = r'''
#include "vm_check_plan.h"
#include <stdio.h>
#include <vector>
int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint32_t h[4];
    while (fread(h, 4, 4, f) == 4) {
        std::vector<uint32_t> w(h[3]);
        if (h[3] && fread(w.data(), 4, h[3], f) != h[3]) return 3;
        printf("%d\n", vmcheck::verify(h[0] != 0, w.data(), w.size(), h[1], h[2]));
    }
    return 0;
}
'''


def _verify(tmp_path, cases):
    src, exe, blob = tmp_path / "driver.cpp", tmp_path / "driver", tmp_path / "cases.bin"
    src.write_text(DRIVER)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)])
    with open(blob, "wb") as f:
        for light, words, n, nout in cases:
            f.write(struct.pack("<4I", int(light), n, nout, len(words)))
            f.write(struct.pack("<%dI" % len(words), *words))
    return [int(x) for x in subprocess.run([str(exe), str(blob)], capture_output=True, text=True, check=True).stdout.split()]


def test_refusals_are_decided_before_the_launch(tmp_path):
    light = set(V.OPS[o] for o in V.LIGHT_OPS)
    cases = [c for c in RF.cases() if c[5] != -1]
    assert sum(1 for c in cases if c[5] == -4) >= 25 and sum(1 for c in cases if c[5] == 0) >= 8
    got = _verify(tmp_path, [(op in light, words, n, nout) for name, op, words, n, nout, want in cases])
    assert [(c[0], g) for c, g in zip(cases, got)] == [(c[0], c[5]) for c in cases]


def test_every_program_of_the_gpu_test_is_accepted(tmp_path):
    cases = []
    for p in V.programs():
        check_at, slot = p.check if p.check else (0, 0)
        for op in p.ops:
            for tpw in V.geometries(p):
                imgs = [p.images[t % p.nimg] for t in range(8)]
                cases.append((op in V.LIGHT_OPS, V.call_words(p.rounds, p.table(), p.nslots, imgs, tpw, check_at, slot), 8, 8 * (p.nslots * 12 + V.TRAILER)))
    progs, data, consts = V.production()
    for name, op, rounds, cuts in progs:
        img = V.production_image(name, op, rounds, data, consts)
        cases.append((op in V.LIGHT_OPS, V.call_words(rounds, data, len(img), [img], 1), 1, len(img) * 12 + V.TRAILER))
    assert _verify(tmp_path, cases) == [0] * len(cases)
