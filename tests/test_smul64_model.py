"""The integer model of the multiplication by a short public scalar (vmgen/smul64_model.py, the specification of
csrc/blsgpu_smul64.hip): the digits reconstruct the weight, the window recurrence equals w x on integers and costs what the
kernel's header says; and the boundary of the new calls -- the header declares them, the prototype table covers them."""
import ctypes
import random

import pytest

from test_abi_and_host import header_declarations
from vmgen import smul64_model as M

NEW_SYMBOLS = ("blsgpu_g1_mul_short", "blsgpu_g2_mul_short", "blsgpu_g1_mul_short_dev", "blsgpu_g2_mul_short_dev",
               "blsgpu_verify_find", "blsgpu_verify_find_dev")


def weights():
    rng = random.Random(0x736d3634)
    fixed = [0, 1, 15, 16, 1 << 63, (1 << 64) - 1,
             0x0123456789abcdef, 0x00000000ffffffff,      # zero nibbles at the top
             0xffff0000ffff0f0f, 0x8000000100000001,      # ... in the middle
             0xfffffffffffffff0, 0x1234567800000000]      # ... at the bottom
    return fixed + [rng.getrandbits(64) for _ in range(200)]


WEIGHTS = weights()


def test_digits_reconstruct_the_weight():
    assert len(WEIGHTS) == 212
    for w in WEIGHTS:
        d = M.digits(w)
        assert len(d) == M.WINDOWS == 16 and all(0 <= x < 16 for x in d)
        assert sum(x << (4 * j) for j, x in enumerate(d)) == w
        assert d == [int(c, 16) for c in reversed("%016x" % w)]
    for bad in (-1, 1 << 64):
        with pytest.raises(ValueError):
            M.digits(bad)


def test_window_recurrence_is_w_times_x():
    rng = random.Random(7)
    xs = [1, 3, (1 << 381) - 19, rng.getrandbits(255)]
    for w in WEIGHTS:
        for x in xs:
            got, ops = M.smul(x, w)
            assert got == w * x, hex(w)
            assert ops == {"dbl": 60, "add": 16, "table_add": 14}
    assert M.build_table(5) == [5 * e for e in range(16)]


def test_header_declares_the_new_calls():
    declared = header_declarations()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert declared[name][0] == "int"
    short = ["pointer", "pointer", "pointer", "size_t", "pointer", "pointer"]
    assert declared["blsgpu_g1_mul_short"][1] == declared["blsgpu_g2_mul_short"][1] == short
    assert declared["blsgpu_g1_mul_short_dev"][1] == declared["blsgpu_g2_mul_short_dev"][1] == short + ["pointer"]
    find = ["pointer", "pointer", "pointer", "size_t", "pointer", "pointer", "size_t", "pointer", "pointer", "size_t", "pointer", "pointer"]
    assert declared["blsgpu_verify_find"][1] == find
    assert declared["blsgpu_verify_find_dev"][1] == find + ["pointer"]


def test_prototype_table_covers_the_new_calls():
    from bls_py import _native, backend

    def kind(t):
        return "pointer" if t in (ctypes.c_void_p, ctypes.c_char_p) else {ctypes.c_size_t: "size_t", ctypes.c_int: "int"}[t]

    declared = header_declarations()
    for name in NEW_SYMBOLS:
        assert name in _native.PROTOTYPES and name in _native.SYMBOLS, name
        assert [kind(t) for t in _native.PROTOTYPES[name]] == declared[name][1], name
    from bls_py import _native_find
    for method in ("g1_mul_short", "g2_mul_short", "verify_find"):
        assert callable(getattr(_native_find, method)) and callable(getattr(_native_find, method + "_dev"))
        assert backend.FIND_EXTENSIONS[method] == "_native_find" and not hasattr(_native.Engine, method)
    p = backend.HipProvider.__new__(backend.HipProvider)
    p._eng = object()
    old = backend._provider
    try:
        backend.use(p)
        fn = backend.extension("verify_find")
        assert fn.func is _native_find.verify_find and fn.args == (p._eng,)
    finally:
        backend.use(old)
