"""GPU: the compiled 32-bit-limb field layer (csrc/fq32.h, csrc/fq_mul_gfx950.h) and the LIN-round helpers of run_rounds
(fat_flip / fat_mac_plain / fat_reduce, lin_absorb of csrc/blsgpu_lin_absorb.h) against Python integers, word for word,
through the test-only library csrc/blsgpu_fq32_check.hip (libblsgpu_fq32check.so: one kernel per primitive, one item per
lane).  This is the layer where the device compiles other code than the host: the inline-assembly product columns, the
device branch of fat_reduce, inv_mad32, the addc / subc builtins, the DPP absorb.  Operand sets, references and the lane
layout are tests/fq32_vectors.py's; tests/test_fq32_vectors_model.py proves those references on the host build.  Every op
runs with 1, 63, 64, 65 and 257 items, one call each; item i is the same operand set in every call.  Every comparison is
exact: the expected words, and on the device's own output the independent integer check of the op, which on a mismatch
decides who is wrong.  A HIP error or a written guard record fails the call."""
import ctypes

import pytest

import checklib
import fq32_vectors as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def check_lib():
    return checklib.load("libblsgpu_fq32check", "blsgpu_fq32_check")


def _group(lib, group):
    checklib.run_group(lib, V, group)


def test_products(check_lib):
    _group(check_lib, "products")


def test_linear(check_lib):
    _group(check_lib, "linear")


def test_fat_and_lin_rounds(check_lib):
    _group(check_lib, "fat")


def test_decisions(check_lib):
    _group(check_lib, "decisions")


def test_inversions(check_lib):
    _group(check_lib, "inversions")


def test_bad_arguments_are_refused(check_lib):
    """sizes that do not match the op, and an unknown op, launch nothing"""
    buf = (ctypes.c_uint32 * 24)()
    out = (ctypes.c_uint32 * 12)()
    assert check_lib(0, buf, 23, 1, out, 12) == -2
    assert check_lib(0, buf, 24, 1, out, 11) == -2
    assert check_lib(0, buf, 24, 0, out, 12) == -2
    assert check_lib(9, buf, 24, 1, out, 12) == -1
