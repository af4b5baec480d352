"""GPU: the compiled lane-pair (ml::sp), lane-quad (ml::sq) and six-lane-team routines of csrc/blsgpu_ml.hip -- the arithmetic of
k_ml_lines2 / k_ml_lines4 and of k_ml_accum / k_ml_merge / k_ml_small -- against the integer model, word for word, through the
test-only library csrc/blsgpu_ml_check.hip (libblsgpu_mlcheck.so: one kernel per op).  Operand sets and expected words are
tests/ml_vectors.py's; tests/test_ml_vectors_model.py checks them on the CPU.  Lane-pair ops run with 1, 31, 32, 33 and 129
items, quad ops with 1, 15, 16, 17 and 65, team ops with 1, 9, 10, 11 and 41 (either side of a wavefront and of a workgroup), and
further calls of the largest count until every set has run; item i is the same set in every call.  No tolerances: every output
word is compared exactly."""
import numpy as np
import pytest

import checklib
import ml_vectors as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def check_lib():
    return checklib.load("libblsgpu_mlcheck", "blsgpu_ml_check")


@pytest.fixture(scope="module")
def ops():
    return V.ops()


def _run(lib, op):
    checklib.run_sets(lib, V, op, op.counts)


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
    call = lambda code, w, n, o: check_lib(code, w.ctypes.data, w.size, n, o.ctypes.data, o.size)
    assert call(op.code, words[:-1], 1, out) == -2
    assert call(op.code, words, 1, out[:-1]) == -2
    assert call(25, words, 1, out) == -1
    bad = words.copy()
    bad[-1] = 6
    assert call(op.code, bad, 1, out) == -4
