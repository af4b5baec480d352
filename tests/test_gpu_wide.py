"""GPU: the compiled step routines of the wide machine (csrc/blsgpu_mlw.hip mlw::, csrc/blsgpu_lsw.hip lsw::,
csrc/blsgpu_fexpw.hip fxw::) against the integer model, word for word, through the test-only library
csrc/blsgpu_wide_check.hip (libblsgpu_widecheck.so: one kernel per op).  Operand sets, records and references are
tests/wide_vectors.py's; tests/test_wide_vectors_model.py checks them on the CPU.  Per lane ops run with 1, 63, 64, 65 and 257
items, per wavefront ops with 1, 3, 4, 5 and 65 wavefronts (and further calls of 65 until every set has run); every output word
is compared exactly -- the stored results, the unchanged rest of the value file and the guards -- except the write sink's."""
import numpy as np
import pytest

import checklib
import wide_vectors as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def check_lib():
    return checklib.load("libblsgpu_widecheck", "blsgpu_wide_check")


@pytest.fixture(scope="module")
def ops():
    return V.ops()


def _run(lib, op):
    checklib.run_sets(lib, V, op, V.N_WAVE_ITEMS if op.wave else V.N_LANE_ITEMS)


def test_per_lane_ops(check_lib, ops):
    for name in ("SRN", "FXW_SCALE_NORM", "STORED_ZERO"):
        _run(check_lib, ops[name])


@pytest.mark.parametrize("name", ["WSTEP_2", "WSTEP_2BS", "WSTEP_1", "WSTEP_1OCT"])
def test_value_file_step(check_lib, ops, name):
    _run(check_lib, ops[name])


def test_four_wavefronts_per_workgroup(check_lib, ops):
    _run(check_lib, ops["WSTEP_2_X4"])
    _run(check_lib, ops["WSTEP_1_X4"])


def test_input_multiples(check_lib, ops):
    """quad_variant / srn / st14 as the kernels call them on their inputs, with k_miller_wide's factors -3 and 3"""
    _run(check_lib, ops["WLOAD"])


def test_steps_with_records_fetched_by_load_rec(check_lib, ops):
    """every kind of MLW_REC, H2CW_REC, G1W_REC through mlw::load_rec (a kind past the table reads kind 0) and of LSW_REC through
    lsw::load_rec<K>: the same expected words as the records packed on the host"""
    names = [n for n in ops if n.startswith("TREC_") or n.startswith("LREC_")]
    assert len(names) == 12
    for name in names:
        _run(check_lib, ops[name])


def test_line_stream_steps(check_lib, ops):
    for name in V.LSHAPES:
        _run(check_lib, ops[name])


def test_final_exponentiation_steps(check_lib, ops):
    for name in ("FXW_STEP_VV", "FXW_STEP_VG", "FXW_VV_CSQ", "FXW_VV_CONJ", "FXW_VG_MUL", "FXW_VG_FROB", "FXW_VG_FROBC", "FXW_TINV"):
        _run(check_lib, ops[name])


def test_bad_arguments_are_refused(check_lib, ops):
    """sizes that do not match the op, an unknown op and a record that names an address outside the value file launch nothing"""
    op = ops["WSTEP_1"]
    words = np.array(op.sets[0][1], dtype=np.int32)
    out = np.zeros(op.wout, dtype=np.int32)
    call = lambda code, w, n, o: check_lib(code, w.ctypes.data, w.size, n, o.ctypes.data, o.size)
    assert call(op.code, words[:-1], 1, out) == -2
    assert call(op.code, words, 1, out[:-1]) == -2
    assert call(9, words, 1, out) == -1
    bad = words.copy()
    bad[V.MVF + 4 * 64 + 5] = 4 * (V.MVF - 64 * (V.L - 1))          # lane 5 stores one slot past the last
    assert call(op.code, bad, 1, out) == -4
    bad = words.copy()
    bad[V.MVF + 7] = 2                                              # not a dword address
    assert call(op.code, bad, 1, out) == -4
