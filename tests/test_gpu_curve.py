"""GPU: the compiled G2 curve arithmetic on lane pairs (sp2) and lane quads (sp4), the group traits SrtG<1> / SrtG<2> and the digit
routines of csrc/blsgpu_msm.hip -- the arithmetic under k_msm_lane2x, k_msm_horner_quads, k_srt_accum and the sorted-bucket folds,
k_pscan_range<2>, k_smul_seg, k_g2_smul and the two cofactor-clearing kernels -- against the limb model, word for word, through the
test-only library csrc/blsgpu_curve_check.hip (libblsgpu_curvecheck.so: one kernel per op).  Operand sets, expected words and the
independent checks are tests/curve_vectors.py's; tests/test_curve_vectors_model.py checks them on the CPU.  Lane-pair ops run with
1, 31, 32, 33 and 129 items, quad ops with 1, 15, 16, 17 and 65, one-lane ops with 1, 63, 64, 65 and 257, and further calls until
every set has run; item i is the same set in every call.  No tolerances: every output word is compared exactly; for a quad op the
words of pair 1 must equal those of pair 0; and once per set the device's OWN words are checked against bls_py.hostmath as a point
(cross-multiplied mod q), as canonical bytes, or as digits that sum to the scalar."""
import numpy as np
import pytest

import checklib
import curve_vectors as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def check_lib():
    return checklib.load("libblsgpu_curvecheck", "blsgpu_curve_check")


@pytest.fixture(scope="module")
def ops():
    return V.ops()


def _run_group(lib, name):
    sel = V.group(name)
    assert sel
    for op in sel:
        checklib.run_sets(lib, V, op, op.counts, checks=True)


def _xor(lib, ops_, name, DEG, counts, offsets):
    class XorOp:
        pass
    op = XorOp()
    op.name, op.code, op.wout = name, {2: 9, 1: 31}[DEG], V.PT if DEG == 2 else V.P1
    for n in counts:
        for off in offsets:
            words, want = V.xor_call(DEG, n, off)
            assert checklib.call(lib, op, words, n, np.int32) == want, (name, n, off)


def test_lane_pair_ops(check_lib, ops):
    _run_group(check_lib, "pair")
    _xor(check_lib, ops, "SRTG2_XOR_LANES", 2, (32, 96), (1, 2, 4, 8, 16))


def test_lane_quad_ops(check_lib, ops):
    """both pairs of a quad end with the same words (every lane stores its own rows in the kernels)"""
    _run_group(check_lib, "quad")
    for op in V.group("quad"):
        for tag, words, want, coords, chk in op.sets:
            assert want[:V.PT] == want[V.PT:], (op.name, tag)


def test_one_lane_ops(check_lib, ops):
    _run_group(check_lib, "lane")
    _xor(check_lib, ops, "SRTG1_XOR_LANES", 1, (64, 192), (1, 2, 4, 8, 16, 32))


def test_chains(check_lib, ops):
    """outputs fed back as inputs: eight additions from infinity (the second a doubling), the Jacobian detour over 1, 2, 16 and 60
    doublings, a cancellation through the detour to (0, 0) and flag 1, and the running sums of k_msm_lane2x"""
    _run_group(check_lib, "chain")


def test_digits(check_lib, ops):
    for op in V.group("digit"):
        checklib.run_sets(check_lib, V, op, op.counts + (len(op.sets),))
    # the device's own digits, put together again: sum d_w 16^w = s (with `big`: plain nibbles)
    op = ops["LANE_DIGIT"]
    scal = V.digit_scalars()
    words = [w for _, s in scal for win in range(64) for w in V.scalar_words(s) + [win]]
    got = checklib.call(check_lib, op, words, 64 * len(scal), np.int32)
    for i, (tag, s) in enumerate(scal):
        d = got[64 * i:64 * i + 64]
        assert len({b for _, b in d}) == 1 and d[0][1] == int((s >> 224) > 0x77777776), tag
        assert sum(x << (4 * w) for w, (x, _) in enumerate(d)) == s, tag
        assert all((0 <= x <= 15) if b else (-8 <= x <= 7) for x, b in d), tag
    # ... and sum (v_w - 2^(cb - 1)) 2^(cb w) = s, key = |d| - 1 and the sign, for every cb
    op = ops["SRT_DIGIT_KEY"]
    for cb in range(5, V.SRT_MAXBITS + 1):
        nw, half = V.srt_windows(cb), 1 << (cb - 1)
        words = [w for _, s in scal for win in range(nw) for w in V.srt_record(s, cb) + [win, cb]]
        got = checklib.call(check_lib, op, words, nw * len(scal), np.int32)
        for i, (tag, s) in enumerate(scal):
            rows = got[nw * i:nw * i + nw]
            assert sum((v - half) << (cb * w) for w, (v, k, sign, nz) in enumerate(rows)) == s, (cb, tag)
            for v, k, sign, nz in rows:
                d = v - half
                assert nz == int(d != 0) and sign == int(d < 0), (cb, tag)
                if d:
                    assert k == abs(d) - 1 and 0 <= k < half, (cb, tag)


def test_bad_arguments_are_refused(check_lib, ops):
    """sizes that do not match the op, an unknown op, and every word a routine would index or shift with launch nothing"""
    def call(code, words, n, wout):
        w, o = np.array(words, dtype=np.int32), np.zeros(wout, dtype=np.int32)
        return check_lib(code, w.ctypes.data, w.size, n, o.ctypes.data, o.size)
    op = ops["SRT_DIGIT_KEY"]
    rec = list(op.sets[0][1][:9])
    assert call(op.code, rec + [0, 5], 1, 4) == 0
    assert call(op.code, rec + [0], 1, 4) == -2 and call(op.code, rec + [0, 5], 1, 3) == -2 and call(19, rec + [0, 5], 1, 4) == -1
    for w, cb in ((0, 4), (0, V.SRT_MAXBITS + 1), (52, 5), (19, 14), (20, 13), (-1, 8)):
        assert call(op.code, rec + [w, cb], 1, 4) == -4, (w, cb)
    assert call(op.code, rec + [51, 5], 1, 4) == 0 and call(op.code, rec + [18, 14], 1, 4) == 0 and call(op.code, rec + [19, 13], 1, 4) == 0
    ld = ops["LANE_DIGIT"]
    assert call(ld.code, list(ld.sets[0][1][:8]) + [64], 1, 2) == -4 and call(61, [64, 0], 1, 1) == -4 and call(61, [3, 1], 1, 1) == -4
    m = ops["SRTG2_MADD"]
    assert call(m.code, list(m.sets[0][1][:-1]) + [2], 1, m.wout) == -4
    a = ops["SRTG1_AFFINE_OUT"]
    assert call(a.code, list(a.sets[0][1][:-1]) + [2], 1, a.wout) == -4
    words, _ = V.xor_call(2, 32, 4)
    assert call(9, words[:31 * (V.PT + 1)], 31, 31 * V.PT) == -4              # not whole wavefronts
    for bad in (0, 3, 32):
        w2 = list(words)
        for i in range(32):
            w2[i * (V.PT + 1) + V.PT] = bad
        assert call(9, w2, 32, 32 * V.PT) == -4, bad
    w2 = list(words)
    w2[-1] = 2                                                                  # one item with another offset
    assert call(9, w2, 32, 32 * V.PT) == -4
