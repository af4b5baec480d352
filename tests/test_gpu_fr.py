"""GPU: the compiled scalar-field and byte-hashing layer (csrc/fr_scalar.h, hd_derive.h, hash_pks.h, sigdiv.h,
secret_window.h) against Python integers, hashlib / hmac and the window models, word for word, through the test-only library
csrc/blsgpu_fr_check.hip (libblsgpu_frcheck.so: one kernel per routine, one item per lane).  The host tests of these headers
say nothing about the gfx950 build, and the API-level GPU tests never choose an operand of frs::mul or frs::inv;
secret_window.h has no host build at all.  Operand sets, references and the lane layout are tests/fr_vectors.py's;
tests/test_fr_vectors_model.py proves those references on the host build and shows that a list of mutants is caught.  Every op
runs with 1, 63, 64, 65 and 257 items, one call each; item i is the same operand set in every call.  Every comparison is
exact: the expected words, and on the device's own output the independent integer check of the op (a a^-1 = 1,
sum d_w 16^w = s, ...), which on a mismatch decides who is wrong.  A HIP error or a written guard record fails the call."""
import ctypes

import pytest

import checklib
import fr_vectors as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def check_lib():
    return checklib.load("libblsgpu_frcheck", "blsgpu_fr_check")


def _group(lib, group):
    checklib.run_group(lib, V, group)


def test_reduce(check_lib):
    _group(check_lib, "reduce")


def test_products(check_lib):
    _group(check_lib, "products")


def test_inversions(check_lib):
    _group(check_lib, "inversions")


def test_lagrange(check_lib):
    _group(check_lib, "lagrange")


def test_sigdiv(check_lib):
    _group(check_lib, "sigdiv")


def test_sha(check_lib):
    _group(check_lib, "sha")


def test_window(check_lib):
    _group(check_lib, "window")


def test_bad_arguments_are_refused(check_lib):
    """sizes that do not match the op, and an unknown op, launch nothing"""
    buf = (ctypes.c_uint32 * 16)()
    out = (ctypes.c_uint32 * 8)()
    mul = V.OPS["mul"].code
    assert check_lib(mul, buf, 15, 1, out, 8) == -2
    assert check_lib(mul, buf, 16, 1, out, 7) == -2
    assert check_lib(mul, buf, 16, 0, out, 8) == -2
    assert check_lib(19, buf, 16, 1, out, 8) == -1
    assert check_lib(-1, buf, 16, 1, out, 8) == -1
