"""GPU: the compiled register layer behind hash to G2, hash to G1 and decompression (csrc/blsgpu_h2c.hip namespace swl -- jacobi, chi, sgn,
red, inv, scale, ldv / stv / st_zero --, the window loop of k_pow and the two-wave base-4 loop of k_pow2, csrc/blsgpu_h2g1.hip's pow_e,
field_element<0 / 1> and sel, and sha256_block) against the limb model, word for word, through the test-only library
csrc/blsgpu_h2c_check.hip (libblsgpu_h2ccheck.so: one kernel per op, one item per lane).  Operand sets, expected words and the independent
checks are tests/h2c_vectors.py's; tests/test_h2c_vectors_model.py checks them on the CPU.  Every op runs with 1, 63, 64, 65 and 257 items
(the two power loops with 1, 63, 64, 65, 127, 128, 129 and 257, so that k_pow2's clamp repeats the last value) and with further calls of the
largest count until every set has run.  No tolerances: every output word is compared exactly, and once per set the device's OWN words are
checked in plain integers (Euler's criterion, pow, a out = 1, int.from_bytes % q, hashlib).

The REAL power kernels run through engines: one with BLSGPU_POW2_MAX = 0 (always k_pow), one with it above any size (always k_pow2), on
the same decompression and map inputs at 1, 63, 65 and 129 items; both must return the same bytes and flags, and the fixtures' bytes."""
import numpy as np
import pytest

import checklib
import h2c_vectors as V
from test_gpu_h2c_forced import CONFIGS, environment, stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def check_lib():
    return checklib.load("libblsgpu_h2ccheck", "blsgpu_h2c_check")


@pytest.fixture(scope="module")
def ops():
    return V.ops()


def _run(lib, op):
    seen, checked = set(), set()

    def one(n, base):
        sets = V.call_sets(op, n, base)
        got = checklib.call(lib, op, [w for k in sets for w in op.sets[k][1]], n, np.int32)
        for i, k in enumerate(sets):
            tag, _, want, chk = op.sets[k]
            where = "%s, %d items, item %d (lane %d), set %s" % (op.name, n, i, i % 64, tag)
            if got[i] != want:
                try:                                   # who is wrong: the independent check on the device's words decides
                    chk(got[i])
                except AssertionError as err:
                    raise AssertionError("%s: the device is wrong (%s)" % (where, err))
                bad = [(j, g, w) for j, (g, w) in enumerate(zip(got[i], want)) if g != w]
                raise AssertionError("%s: device and model differ in %d words, first (word, got, want) %s" % (where, len(bad), bad[:4]))
            if k not in checked:
                checked.add(k)
                chk(got[i])
        seen.update(sets)

    for n in op.counts:
        one(n, 0)
    step = (op.counts[-1] + 63) // 64 if op.wave else op.counts[-1]
    base = step
    while len(seen) < len(op.sets):
        assert base < 64 * step, op.name
        one(op.counts[-1], base)
        base += step


def test_binary_jacobi(check_lib, ops):
    """swl::jacobi itself: corners, 2^k and 2^k +- 1 up to k = 380, both characters of every residue mod 8, the longest runs"""
    _run(check_lib, ops["JACOBI_BIN"])


def test_chi_in_every_form(check_lib, ops):
    _run(check_lib, ops["CHI"])


def test_sign_at_the_half_and_in_every_form(check_lib, ops):
    _run(check_lib, ops["SGN"])


def test_red_inv_scale(check_lib, ops):
    """inv: 0 -> 0, a value per lane with zeros beside non-zero values, and one value per wavefront"""
    for name in ("RED_02", "RED_11", "INV", "INV_WAVE", "SCALE"):
        _run(check_lib, ops[name])


def test_image_slots(check_lib, ops):
    """stv, ldv, stv and st_zero at the lowest and highest slot the kernels name; every other word of the image untouched"""
    _run(check_lib, ops["LDV_STV"])


def test_pow_e(check_lib, ops):
    _run(check_lib, ops["POW_E"])


def test_power_loops(check_lib, ops):
    """the window loop of k_pow and the base-4 loop of k_pow2 on the same bases: the same words from both"""
    a, b = ops["POW_LOOP_WIN"], ops["POW_LOOP_B4"]
    assert [s[:2] for s in a.sets] == [s[:2] for s in b.sets]
    assert [s[2][V.L:] for s in a.sets] == [s[2][V.L:] for s in b.sets]      # canonical words agree (the limbs need not)
    _run(check_lib, a)
    _run(check_lib, b)


def test_field_elements_sel_sha(check_lib, ops):
    for name in ("FIELD_ELEMENT_0", "FIELD_ELEMENT_1", "FE1_REDUCE", "SEL", "SHA256_BLOCK"):
        _run(check_lib, ops[name])


def test_bad_arguments_are_refused(check_lib, ops):
    """sizes that do not match the op, an unknown op, an image slot outside [STATE0, STATE1) launch nothing"""
    def call(code, words, n, wout):
        w, o = np.array(words, dtype=np.int32), np.zeros(wout, dtype=np.int32)
        return check_lib(code, w.ctypes.data, w.size, n, o.ctypes.data, o.size)
    op = ops["LDV_STV"]
    words = list(op.sets[0][1])
    assert call(op.code, words, 1, op.wout) == 0
    assert call(op.code, words[:-1], 1, op.wout) == -2 and call(op.code, words, 1, op.wout - 1) == -2 and call(op.code, words, 0, op.wout) == -2
    assert call(8, words, 1, op.wout) == -1 and call(25, words, 1, op.wout) == -1
    for at in range(3):
        for bad in (V.STATE0 - 1, V.STATE1, -1, 1 << 30):
            assert call(op.code, words[:at] + [bad] + words[at + 1:], 1, op.wout) == -4, (at, bad)
    assert call(op.code, words + [V.STATE1] + words[1:], 2, 2 * op.wout) == -4


# ---- the real power kernels: k_pow against k_pow2 ---------------------------------------------------------------------------------
BIG = str(1 << 40)
_engines = {}


def _engine(config, pow2_max):
    from bls_py import _native
    key = (config, pow2_max)
    if key not in _engines:
        with environment(dict(CONFIGS[config], BLSGPU_POW2_MAX=pow2_max)):
            _engines[key] = _native.Engine(0)
    return _engines[key]


COUNTS = (1, 63, 65, 129)


def test_decompression_k_pow_against_k_pow2():
    import random
    Q = V.Q
    rng = random.Random(21)                            # the encodings of test_gpu_decompress.py::test_random_and_rejected_encodings
    enc1 = [bytes([rng.randrange(256) for _ in range(48)]) for _ in range(300)]
    enc2 = [bytes([rng.randrange(256) for _ in range(96)]) for _ in range(150)]
    enc1 += [bytes(48), b"\x80" + bytes(47), b"\xff" * 48, (Q + 5).to_bytes(48, "big")]
    enc2 += [bytes(96), b"\x80" + bytes(95), b"\xff" * 96, bytes(47) + b"\x01" + bytes(48), bytes(95) + b"\x01"]
    from test_gpu_decompress import compare
    a, b = _engine("vm+vm", "0"), _engine("vm+vm", BIG)
    for n in COUNTS:
        for encs, fn in ((enc1[-n:], "g1_decompress"), (enc2[-n:], "g2_decompress")):
            ra, rb = getattr(a, fn)(b"".join(encs)), getattr(b, fn)(b"".join(encs))
            assert ra == rb, (fn, n)
    compare(a, 1, enc1)
    compare(a, 2, enc2)
    compare(b, 1, enc1)
    compare(b, 2, enc2)


def test_g2_real_u_decompression_k_pow_against_k_pow2(golden):
    recs = golden("g2_real_u.json")["decompress"]
    encs = b"".join(bytes.fromhex(r["encoding"]) for r in recs)
    ra, rb = _engine("vm+vm", "0").g2_decompress(encs), _engine("vm+vm", BIG).g2_decompress(encs)
    assert ra == rb and not any(ra[1])


@pytest.mark.parametrize("config", ["vm+vm", "jacobi+pairs"])
def test_map_to_g2_k_pow_against_k_pow2(config, golden):
    items = [(bytes.fromhex(r["t"]) + bytes(96), None) for r in golden("hash_to_curve.json")["sw_encode_fq2"]]
    for fixture, key in (("g2_real_u.json", "sw_encode"), ("h2c_corners.json", "cases")):
        items += [(bytes.fromhex(r["t"]), r["point"]) for r in golden(fixture)[key]]
    # the padding up to 129 items is raw hash output ON PURPOSE: most of its 48-byte coordinates are at or above q (t is taken mod q, any value
    # below 2^384 is admitted), which no other test feeds map_to_g2; no fixture knows their points, the two engines must agree on them
    items += [(t, None) for t in stream(b"blsgpu/h2c-check", 129 - len(items), 192)] if len(items) < 129 else []
    a, b = _engine(config, "0"), _engine(config, BIG)
    for n in COUNTS:
        part = items[:n] if n < len(items) else items
        t = b"".join(x for x, _ in part)
        oa, ob = a.map_to_g2(t), b.map_to_g2(t)
        assert oa == ob, (config, n)
        for i, (_, want) in enumerate(part):
            if want is not None:
                assert oa[192 * i:192 * (i + 1)].hex() == want, (config, n, i)
    # the fixtures that record a point, whatever the count left of them: the last items as well
    tail = [it for it in items if it[1] is not None]
    for e in (a, b):
        out = e.map_to_g2(b"".join(x for x, _ in tail))
        assert [out[192 * i:192 * (i + 1)].hex() for i in range(len(tail))] == [w for _, w in tail]
    vec = golden("hash_to_curve.json")["hash_to_g2"]
    msgs = b"".join(bytes.fromhex(r["msg_hash"]) for r in vec)
    assert a.hash_to_g2(msgs) == b.hash_to_g2(msgs) == bytes.fromhex("".join(r["point"] for r in vec))
