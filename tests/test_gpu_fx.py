"""GPU: the compiled steps of the six-lanes-per-result final exponentiation (csrc/blsgpu_fexp.hip, namespace fx: reduce_small, cyc_sqr,
frob, tinv, fq_inverse, and k_fexp_team's inline CONJ and slot traffic) against the limb model, word for word, through the test-only
library csrc/blsgpu_fx_check.hip (libblsgpu_fxcheck.so: one kernel per op).  Operand sets, expected words and the independent checks
are tests/fx_vectors.py's; tests/test_fx_vectors_model.py checks them on the CPU.  Team ops run with 1, 9, 10, 11 and 41 items, per-lane
ops with 1, 63, 64, 65 and 257, and further calls of the largest count until every set has run; item i is the same set in every call,
so the teams of a wavefront all differ.  No tolerances: every output word is compared exactly, and once per set the device's OWN words
are checked in plain integers mod q.  One test runs the PRODUCT: k_fexp_team with its trace buffer, compared with
vmgen/fexp_model's interpreter after every script entry."""
import numpy as np
import pytest

import checklib
import fx_vectors as V
from vmgen import fexp_model as F

pytestmark = pytest.mark.gpu
Q = V.Q


@pytest.fixture(scope="module")
def check_lib():
    return checklib.load("libblsgpu_fxcheck", "blsgpu_fx_check")


@pytest.fixture(scope="module")
def ops():
    return V.ops()


def _run(lib, op):
    checklib.run_sets(lib, V, op, op.counts, checks=True)


def test_reduce_small(check_lib, ops):
    """every multiple of q it is claimed for, both sides of every point where the float estimate changes k, tops past 2^24"""
    _run(check_lib, ops["REDUCE_SMALL"])


def test_fermat_inverse(check_lib, ops):
    """the BLSGPU_FEXP_FERMAT branch of tinv, which no production build compiles: a zero beside non-zero lanes"""
    _run(check_lib, ops["FQ_INVERSE"])


def test_cyclotomic_squaring(check_lib, ops):
    _run(check_lib, ops["CYC_SQR"])


def test_cyclotomic_squaring_chains(check_lib, ops):
    """the kernel's run-time loop: n = 1, 2, the script's longest run and one more, from cyclotomic values, from 1, from extreme digits"""
    op = ops["CYC_SQR_CHAIN"]
    assert sorted(op.by_n) == [1, 2, V.longest_run(), V.longest_run() + 1]
    _run(check_lib, op)


def test_frobenius_maps(check_lib, ops):
    _run(check_lib, ops["FROB"])


def test_fq2_inversion(check_lib, ops):
    _run(check_lib, ops["TINV"])


def test_conjugation_and_slot_roundtrip(check_lib, ops):
    _run(check_lib, ops["CONJ"])
    _run(check_lib, ops["SLOT_ROUNDTRIP"])


def test_bad_arguments_are_refused(check_lib, ops):
    """sizes that do not match the op, an unknown op, a chain count or a Frobenius index that is too large or not uniform launch nothing"""
    def call(code, words, n, wout):
        w, o = np.array(words, dtype=np.int32), np.zeros(wout, dtype=np.int32)
        return check_lib(code, w.ctypes.data, w.size, n, o.ctypes.data, o.size)
    op = ops["FROB"]
    words = list(op.sets[0][1])
    assert call(op.code, words, 1, op.wout) == 0
    assert call(op.code, words[:-1], 1, op.wout) == -2 and call(op.code, words, 1, op.wout - 1) == -2 and call(op.code, words, 0, op.wout) == -2
    assert call(5, words, 1, op.wout) == -1 and call(16, words, 1, op.wout) == -1
    for bad in (3, -1, 255):
        assert call(op.code, words[:-1] + [bad], 1, op.wout) == -4, bad
    assert call(op.code, words[:-1] + [1] + words[:-1] + [2], 2, 2 * op.wout) == -4
    ch = ops["CYC_SQR_CHAIN"]
    words = list(ch.sets[0][1])
    assert call(ch.code, words[:-1] + [V.MAX_CHAIN], 1, ch.wout) == 0
    for bad in (V.MAX_CHAIN + 1, -1, 1 << 20):
        assert call(ch.code, words[:-1] + [bad], 1, ch.wout) == -4, bad
    assert call(ch.code, words[:-1] + [1] + words[:-1] + [2], 2, 2 * ch.wout) == -4


def _trace_inputs(golden):
    import random
    rnd = random.Random("fx:trace")
    z = (0, 0)
    g = golden("pairing.json")
    ints = lambda b: [int.from_bytes(b[48 * i:48 * (i + 1)], "big") for i in range(12)]
    out = [("generator-miller", F.from_flat12(ints(bytes.fromhex(g["gen"]["miller"])))),
           ("zero", [z] * 6), ("one", [(1, 0)] + [z] * 5), ("minus-one", [(Q - 1, 0)] + [z] * 5),
           ("fq2", [(rnd.randrange(Q), rnd.randrange(Q))] + [z] * 5),
           ("fq6", [(rnd.randrange(Q), rnd.randrange(Q)) if k % 2 == 0 else z for k in range(6)])]
    out += [("w%d" % k, [(1, 0) if c == k else z for c in range(6)]) for k in range(1, 6)]
    out += [("all-q-1", [(Q - 1, Q - 1)] * 6), ("cyclotomic", V.cyclotomic_of(V.rnd_val(rnd)))]
    return out


def test_every_script_entry_through_the_product(golden):
    """tools/fexp_trace.py as an assertion: k_fexp_team (the team path forced on an engine of its own) writes result 0's accumulator
    after EVERY script entry; each is compared with vmgen/fexp_model's interpreter (after TINV coefficient 0 only, as the tool does).
    The only cover of the script dispatch, ST / LD and the kernel's own slot indexing."""
    import torch
    from bls_py import _native
    S = F.script()
    e = _native.Engine(0)
    try:
        e.set_fexp_team_threshold(1)
        buf = torch.zeros(len(S) * 576, dtype=torch.uint8, device="cuda")
        e._check(e.lib.blsgpu_ctx_set_fexp_trace(e.h, buf.data_ptr()), "trace")
        try:
            for name, f in _trace_inputs(golden):
                buf.zero_()
                x = b"".join(v.to_bytes(48, "big") for v in F.to_flat12(f))
                out = e.final_exp(x)
                torch.cuda.synchronize()
                tr = bytes(buf.cpu().numpy())
                ints = lambda b: [int.from_bytes(b[48 * i:48 * (i + 1)], "big") for i in range(12)]
                M, acc, n = [None] * F.NSLOTS, list(f), 0
                for pc, (op, a) in enumerate(S):
                    if op == F.MUL:
                        acc = F.mul_dense(acc, M[a])
                    elif op == F.CSQ:
                        for _ in range(a):
                            acc = F.cyc_sqr_lane_forms(acc)
                    elif op == F.ST:
                        M[a] = list(acc)
                    elif op == F.LD:
                        acc = list(M[a])
                    elif op == F.CONJ:
                        acc = F.conj6(acc)
                    elif op == F.FROB:
                        acc = F.frob(acc, F.FROB_POW[a])
                    elif op == F.TINV:
                        t = acc[0]
                        ni = F.fq_inv((t[0] * t[0] + t[1] * t[1]) % Q)
                        acc = [(t[0] * ni % Q, (-t[1]) * ni % Q)] + [(0, 0)] * 5
                    else:
                        break
                    got = F.from_flat12(ints(tr[576 * pc:576 * (pc + 1)]))
                    if op == F.TINV:
                        assert got[0] == acc[0], (name, pc)
                    else:
                        bad = [k for k in range(6) if got[k] != acc[k]]
                        assert not bad, "%s: after entry %d (op %d, arg %d) coefficients %s differ" % (name, pc, op, a, bad)
                    n += 1
                assert n == len(S) - 1
                assert out == b"".join(v.to_bytes(48, "big") for v in F.to_flat12(acc)), name
        finally:
            e._check(e.lib.blsgpu_ctx_set_fexp_trace(e.h, None), "trace off")
    finally:
        e.close()
