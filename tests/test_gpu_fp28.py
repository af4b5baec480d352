"""GPU: the compiled 28-bit-limb field layer (csrc/fp28.h, csrc/fp28_mul_gfx950.h) against the integer model, limb for
limb, through the test-only library csrc/blsgpu_fp28_check.hip (libblsgpu_fp28check.so: one kernel per primitive, one item
per lane).  Operand sets, references and the lane layout are tests/fp28_vectors.py's; tests/test_fp28_vectors_model.py
checks those references on the CPU.  Every op runs with 1, 63, 64, 65 and 257 items, one call each; item i is the same
operand set in every call.  Every comparison is exact: the expected words from the model, and on the device's own
output the independent integer / hostmath check of the op.  A HIP error or a written guard record fails the call."""
import ctypes

import numpy as np
import pytest

import checklib
import fp28_vectors as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def check_lib():
    return checklib.load("libblsgpu_fp28check", "blsgpu_fp28_check")


def _item_call(name, n):
    """V.call_words and V.expected in the form of the other lane-layout modules' V.call"""
    op, want = V.OPS[name], V.expected(name)
    words, idx = V.call_words(name, n)
    chk = [(lambda g, w=op.sets[k][1]: op.check(w, g)) if op.check is not None else None for k in idx]
    return words, idx, [want[k] for k in idx], chk


def _group(lib, group):
    checklib.run_group(lib, V, group, np.int32, _item_call)


def test_raw_products(check_lib):
    _group(check_lib, "raw")


def test_linear_and_carry(check_lib):
    _group(check_lib, "linear")


def test_typed_products(check_lib):
    _group(check_lib, "typed")


def test_boundaries(check_lib):
    _group(check_lib, "boundary")


def test_fq2(check_lib):
    _group(check_lib, "fq2")


def test_curve(check_lib):
    _group(check_lib, "curve")


def test_bad_arguments_are_refused(check_lib):
    """sizes that do not match the op, and an unknown op, launch nothing"""
    buf = (ctypes.c_int32 * 28)()
    out = (ctypes.c_int32 * 14)()
    assert check_lib(0, buf, 27, 1, out, 14) == -2
    assert check_lib(0, buf, 28, 1, out, 13) == -2
    assert check_lib(9, buf, 28, 1, out, 14) == -1
