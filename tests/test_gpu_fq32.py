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
import os

import pytest

import fq32_vectors as V

pytestmark = pytest.mark.gpu

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "python-bls_amd", "csrc", "libblsgpu_fq32check.so")


@pytest.fixture(scope="module")
def check_lib():
    import torch  # noqa: F401  (first, as bls_py._native.load_library: both bind to one HIP runtime)
    assert os.path.exists(LIB), "libblsgpu_fq32check.so is not built: run __graft_entry__.build() (make -C python-bls_amd/csrc)"
    lib = ctypes.CDLL(LIB)
    lib.blsgpu_fq32_check.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t, ctypes.c_size_t,
                                      ctypes.POINTER(ctypes.c_uint32), ctypes.c_size_t]
    lib.blsgpu_fq32_check.restype = ctypes.c_int
    return lib


def _run(lib, op, n, words):
    cin = (ctypes.c_uint32 * len(words))(*words)
    cout = (ctypes.c_uint32 * (n * op.wout))()
    rc = lib.blsgpu_fq32_check(op.code, cin, len(words), n, cout, n * op.wout)
    assert rc == 0, "%s, %d items: blsgpu_fq32_check returned %d (-3: a guard record was written; > 0: HIP error)" % (op.name, n, rc)
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
                if n == V.N_ITEMS[-1] and c is not None and (op.wave or k not in checked):
                    checked.add(k)
                    c(g)
            if n == V.N_ITEMS[-1]:
                assert set(idx) == set(range(len(op.sets))), op.name
            ran += 1
    assert ran


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
    assert check_lib.blsgpu_fq32_check(0, buf, 23, 1, out, 12) == -2
    assert check_lib.blsgpu_fq32_check(0, buf, 24, 1, out, 11) == -2
    assert check_lib.blsgpu_fq32_check(0, buf, 24, 0, out, 12) == -2
    assert check_lib.blsgpu_fq32_check(9, buf, 24, 1, out, 12) == -1
