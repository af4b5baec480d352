"""GPU: the compiled lane-pair (ml::sp), lane-quad (ml::sq) and six-lane-team routines of csrc/blsgpu_ml.hip -- the arithmetic of
k_ml_lines2 / k_ml_lines4 and of k_ml_accum / k_ml_merge / k_ml_small -- against the integer model, word for word, through the
test-only library csrc/blsgpu_ml_check.hip (libblsgpu_mlcheck.so: one kernel per op).  Operand sets and expected words are
tests/ml_vectors.py's; tests/test_ml_vectors_model.py checks them on the CPU.  Lane-pair ops run with 1, 31, 32, 33 and 129
items, quad ops with 1, 15, 16, 17 and 65, team ops with 1, 9, 10, 11 and 41 (either side of a wavefront and of a workgroup), and
further calls of the largest count until every set has run; item i is the same set in every call.  No tolerances: every output
word is compared exactly."""
import ctypes
import os

import numpy as np
import pytest

import ml_vectors as V

pytestmark = pytest.mark.gpu

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "python-bls_amd", "csrc", "libblsgpu_mlcheck.so")


@pytest.fixture(scope="module")
def check_lib():
    import torch  # noqa: F401  (first, as bls_py._native.load_library: both bind to one HIP runtime)
    assert os.path.exists(LIB), "libblsgpu_mlcheck.so is not built: run __graft_entry__.build() (make -C python-bls_amd/csrc)"
    lib = ctypes.CDLL(LIB)
    lib.blsgpu_ml_check.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
    lib.blsgpu_ml_check.restype = ctypes.c_int
    return lib


@pytest.fixture(scope="module")
def ops():
    return V.ops()


def _call(lib, op, sets):
    n = len(sets)
    cin = np.array([w for k in sets for w in op.sets[k][1]], dtype=np.int32)
    cout = np.zeros(n * op.wout, dtype=np.int32)
    rc = lib.blsgpu_ml_check(op.code, cin.ctypes.data, cin.size, n, cout.ctypes.data, cout.size)
    assert rc == 0, "%s, %d items: blsgpu_ml_check returned %d (-3: a guard record was written; > 0: HIP error)" % (op.name, n, rc)
    got = cout.reshape(n, op.wout)
    for i, k in enumerate(sets):
        tag, _, want, _ = op.sets[k]
        if (got[i] == np.array(want, dtype=np.int32)).all():
            continue
        g = got[i].tolist()
        bad = [(j, g[j], w) for j, w in enumerate(want) if g[j] != w]
        assert not bad, "%s, %d items, item %d, set %s: %d words differ, first (word, got, want) %s" % (op.name, n, i, tag, len(bad), bad[:4])


def _run(lib, op):
    counts = op.counts
    seen = set()
    for n in counts:
        sets = V.call_sets(op, n)
        _call(lib, op, sets)
        seen |= set(sets)
    base = counts[-1]
    while len(seen) < len(op.sets):                # the sets a call of the largest count has not reached yet
        sets = V.call_sets(op, counts[-1], base)
        _call(lib, op, sets)
        seen |= set(sets)
        base += counts[-1]


def test_lane_pair_linear_and_carry_ops(check_lib, ops):
    for name in ("MUL_XI", "B3", "NORM_2", "NORM_4", "MULC_NORM_4_S3", "MULC_NORM_3_S2", "MULC_NORM_12_S2", "MULC_NORM_N12_S2"):
        _run(check_lib, ops[name])


def test_lane_pair_products(check_lib, ops):
    for name in ("MUL_31", "MUL_11", "DOT2_1111", "SQR_H", "SQR_HN2", "SQR_M12SQR", "MULF_1", "MULF_3"):
        _run(check_lib, ops[name])


def test_lane_pair_zero_test_load_and_store(check_lib, ops):
    _run(check_lib, ops["IS_ZERO2"])
    _run(check_lib, ops["LOAD_STORE"])


@pytest.mark.parametrize("name", ["SP_TANGENT", "SP_CHORD"])
def test_lane_pair_step(check_lib, ops, name):
    _run(check_lib, ops[name])


def test_lane_quad_moves(check_lib, ops):
    _run(check_lib, ops["OTH"])
    _run(check_lib, ops["PICK"])


def test_lane_quad_tangent_step(check_lib, ops):
    _run(check_lib, ops["SQ_TANGENT"])


def test_team_publish_and_fetch(check_lib, ops):
    for name in ("SET_ONE", "PUBLISH_RAW", "PUBLISH_NORM", "FETCH_0", "FETCH_1", "FETCH_2", "FETCH_3", "FETCH_4", "FETCH_5", "FETCH2_RT"):
        _run(check_lib, ops[name])


def test_team_three_term_sums(check_lib, ops):
    for name in ("MUL3_012", "MUL3_345", "MUL3_012_RAW"):
        _run(check_lib, ops[name])


def test_team_sparse_line_product(check_lib, ops):
    """mul_line_k3 at the positions (2, 3), (3, 5) and (4, 5), the column of P3 filled by the extreme sets"""
    _run(check_lib, ops["TEAM_LINE"])


def test_team_dense_products(check_lib, ops):
    for name in ("TEAM_DENSE", "TEAM_SQUARE", "TEAM_TEAMREC"):
        _run(check_lib, ops[name])


def test_bad_arguments_are_refused(check_lib, ops):
    """sizes that do not match the op, an unknown op and a position that is no power of w launch nothing"""
    op = ops["TEAM_LINE"]
    words = np.array(op.sets[0][1], dtype=np.int32)
    out = np.zeros(op.wout, dtype=np.int32)
    call = lambda code, w, n, o: check_lib.blsgpu_ml_check(code, w.ctypes.data, w.size, n, o.ctypes.data, o.size)
    assert call(op.code, words[:-1], 1, out) == -2
    assert call(op.code, words, 1, out[:-1]) == -2
    assert call(25, words, 1, out) == -1
    bad = words.copy()
    bad[-1] = 6
    assert call(op.code, bad, 1, out) == -4
