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
import os

import pytest

import fr_vectors as V

pytestmark = pytest.mark.gpu

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "python-bls_amd", "csrc", "libblsgpu_frcheck.so")


@pytest.fixture(scope="module")
def check_lib():
    import torch  # noqa: F401  (first, as bls_py._native.load_library: both bind to one HIP runtime)
    assert os.path.exists(LIB), "libblsgpu_frcheck.so is not built: run __graft_entry__.build() (make -C python-bls_amd/csrc)"
    lib = ctypes.CDLL(LIB)
    lib.blsgpu_fr_check.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t, ctypes.c_size_t,
                                    ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t]
    lib.blsgpu_fr_check.restype = ctypes.c_int
    return lib


def _run(lib, op, n, words):
    cin = (ctypes.c_uint32 * len(words))(*words)
    cout = (ctypes.c_uint32 * (n * op.wout))()
    rc = lib.blsgpu_fr_check(op.code, cin, len(words), n, cout, n * op.wout)
    assert rc == 0, "%s, %d items: blsgpu_fr_check returned %d (-3: a guard record was written; > 0: HIP error)" % (op.name, n, rc)
    out = list(cout)
    return [out[i * op.wout:(i + 1) * op.wout] for i in range(n)]


def _group(lib, group):
    ran = 0
    for op in V.OPS.values():
        if op.group != group:
            continue
        for n in V.N_ITEMS:
            words, idx, want, chk = V.call(op.name, n)
            got = _run(lib, op, n, words)
            checked = set()
            for i, (k, g, e, c) in enumerate(zip(idx, got, want, chk)):
                where = "%s, %d items, item %d (lane %d), set %d of class %s" % (op.name, n, i, i % 64, k, op.sets[k][0])
                if g != e:
                    # who is wrong: the independent check on the device's words decides (it raises if they are)
                    if c is not None:
                        try:
                            c(g)
                        except AssertionError as err:
                            raise AssertionError("%s: the device is wrong (%s)\n got  %s\n want %s" % (where, err, g, e))
                    raise AssertionError("%s: device and reference differ\n got  %s\n want %s" % (where, g, e))
                if n == V.N_ITEMS[-1] and c is not None and k not in checked:
                    checked.add(k)
                    c(g)
            if n == V.N_ITEMS[-1]:
                assert set(idx) == set(range(len(op.sets))), op.name
            ran += 1
    assert ran and ran % len(V.N_ITEMS) == 0


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
    assert check_lib.blsgpu_fr_check(mul, buf, 15, 1, out, 8) == -2
    assert check_lib.blsgpu_fr_check(mul, buf, 16, 1, out, 7) == -2
    assert check_lib.blsgpu_fr_check(mul, buf, 16, 0, out, 8) == -2
    assert check_lib.blsgpu_fr_check(19, buf, 16, 1, out, 8) == -1
    assert check_lib.blsgpu_fr_check(-1, buf, 16, 1, out, 8) == -1
