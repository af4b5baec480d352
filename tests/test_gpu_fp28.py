"""GPU: the compiled 28-bit-limb field layer (csrc/fp28.h, csrc/fp28_mul_gfx950.h) against the integer model, limb for
limb, through the test-only library csrc/blsgpu_fp28_check.hip (libblsgpu_fp28check.so: one kernel per primitive, one item
per lane).  Operand sets, references and the lane layout are tests/fp28_vectors.py's; tests/test_fp28_vectors_model.py
checks those references on the CPU.  Every op runs with 1, 63, 64, 65 and 257 items, one call each; item i is the same
operand set in every call.  Every comparison is exact: the expected words from the model, and on the device's own
output the independent integer / hostmath check of the op.  A HIP error or a written guard record fails the call."""
import ctypes
import os

import pytest

import fp28_vectors as V

pytestmark = pytest.mark.gpu

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "python-bls_amd", "csrc", "libblsgpu_fp28check.so")


@pytest.fixture(scope="module")
def check_lib():
    import torch  # noqa: F401  (first, as bls_py._native.load_library: both bind to one HIP runtime)
    assert os.path.exists(LIB), "libblsgpu_fp28check.so is not built: run __graft_entry__.build() (make -C python-bls_amd/csrc)"
    lib = ctypes.CDLL(LIB)
    lib.blsgpu_fp28_check.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_size_t, ctypes.c_size_t,
                                      ctypes.POINTER(ctypes.c_int32), ctypes.c_size_t]
    lib.blsgpu_fp28_check.restype = ctypes.c_int
    return lib


def _run(lib, op, n):
    words, idx = V.call_words(op.name, n)
    cin = (ctypes.c_int32 * len(words))(*words)
    cout = (ctypes.c_int32 * (n * op.wout))()
    rc = lib.blsgpu_fp28_check(op.code, cin, len(words), n, cout, n * op.wout)
    assert rc == 0, "%s, %d items: blsgpu_fp28_check returned %d (-3: a guard record was written; > 0: HIP error)" % (op.name, n, rc)
    out = list(cout)
    return idx, [out[i * op.wout:(i + 1) * op.wout] for i in range(n)]


def _group(lib, group):
    ran = 0
    for op in V.OPS.values():
        if op.group != group:
            continue
        want = V.expected(op.name)
        for n in V.N_ITEMS:
            idx, got = _run(lib, op, n)
            checked = set()
            for i, (k, g) in enumerate(zip(idx, got)):
                cls, w = op.sets[k]
                where = "%s, %d items, item %d (lane %d), set %d of class %s" % (op.name, n, i, i % 64, k, cls)
                if g != want[k]:
                    # who is wrong: the independent check on the device's words decides (it raises if they are)
                    if op.check is not None:
                        try:
                            op.check(w, g)
                        except AssertionError as err:
                            raise AssertionError("%s: the device is wrong (%s)\n got  %s\n want %s" % (where, err, g, want[k]))
                    raise AssertionError("%s: device and model differ\n got  %s\n want %s" % (where, g, want[k]))
                if n == V.N_ITEMS[-1] and k not in checked and op.check is not None:
                    checked.add(k)
                    op.check(w, g)
            if n == V.N_ITEMS[-1]:
                assert set(idx) == set(range(len(op.sets))), op.name
            ran += 1
    assert ran


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
    assert check_lib.blsgpu_fp28_check(0, buf, 27, 1, out, 14) == -2
    assert check_lib.blsgpu_fp28_check(0, buf, 28, 1, out, 13) == -2
    assert check_lib.blsgpu_fp28_check(9, buf, 28, 1, out, 14) == -1
