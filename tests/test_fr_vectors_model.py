"""CPU: the operand sets of tests/fr_vectors.py (a) through the HOST build of the op bodies of csrc/blsgpu_fr_check.hip -- the
same records, the same calls into fr_scalar.h / hd_derive.h / hash_pks.h / sigdiv.h with HD_FN = static inline -- against the
Python references the GPU test uses: the proof of the references before a GPU sees them; the `window` group, which has no
host build, against vmgen.g2smul_model / vmgen.g1fixs_model and the digit identity; (b) inside the preconditions each set
claims, with the properties the sets found by emulation were found for; (c) mutants: each of twelve mutations of a reference
differs from the true reference on some set of EVERY op it belongs to.  Needs no GPU."""
import hashlib
import os
import subprocess

import pytest

import fr_vectors as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "python-bls_amd", "csrc")
N, R, M32 = V.N, V.R, V.M32

HOST_DRIVER = r'''
#include "blsgpu_fr_check.hip"
#include <stdio.h>
#include <vector>
int main() {
    int op, win, wout, n;
    while (scanf("%d %d %d %d", &op, &win, &wout, &n) == 4) {
        std::vector<uint32_t> in(win), out(wout);
        for (int i = 0; i < n; i++) {
            for (int j = 0; j < win; j++) if (scanf("%x", &in[j]) != 1) return 1;
            for (int j = 0; j < wout; j++) out[j] = 0xAAAAAAAAu;
            if (!frcheck_host(op, in.data(), out.data())) return 2;
            for (int j = 0; j < wout; j++) printf("%08x ", out[j]);
            printf("\n");
        }
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def host_outputs(tmp_path_factory):
    """every set of every host-compilable op through the host build, one process: {op name: [output words per set]}"""
    d = tmp_path_factory.mktemp("frhost")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(HOST_DRIVER)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", CSRC, "-o", str(exe), str(src)])
    ops = [op for op in V.OPS.values() if op.host]
    lines = []
    for op in ops:
        lines.append("%d %d %d %d" % (op.code, op.win, op.wout, len(op.sets)))
        lines += [" ".join("%x" % w for w in ws) for _, ws in op.sets]
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    res, at = {}, 0
    for op in ops:
        res[op.name] = [[int(x, 16) for x in out[at + i].split()] for i in range(len(op.sets))]
        at += len(op.sets)
        assert all(len(r) == op.wout for r in res[op.name]), op.name
    return res


@pytest.mark.parametrize("group", [g for g in V.GROUPS if g != "window"])
def test_host_build_matches_the_references(host_outputs, group):
    """(a) word for word, and the independent integer check on the expected words"""
    n = 0
    for op in V.OPS.values():
        if op.group != group:
            continue
        assert op.host, op.name
        want = V.expected(op.name)
        for k, ((cls, w), e, g) in enumerate(zip(op.sets, want, host_outputs[op.name])):
            if op.check is not None:
                op.check(w, e)
            assert g == e, "%s, set %d of class %s: host build and reference differ\n got  %s\n want %s" % (op.name, k, cls, g, e)
            n += 1
    assert n


def test_window_references_against_the_models():
    """the group without a host build: both Python models, the digit identity, the range of the top digit, the selects"""
    from vmgen import g1fixs_model, g2smul_model
    import test_g2smul_model
    assert V.g2smul_scalars() == test_g2smul_model.SCALARS
    assert g2smul_model.WINDOWS == V.DIGITS and g1fixs_model.ENTRY_BYTES == 4 * V.G1_DW
    scalars = {}
    for name in ("recode_g1", "recode_g2"):
        op = V.OPS[name]
        top = set()
        for (cls, w), e in zip(op.sets, V.expected(name)):
            s = V.from_be_words(w)
            d = g2smul_model.recode(s)
            assert d == g1fixs_model.recode(s) and e == V.digit_words(d) and all(-8 <= x < 8 for x in d)
            assert sum(x << (4 * i) for i, x in enumerate(d)) == s
            op.check(w, e)
            top.add(d[64])
        assert top == {0, 1}, "the top digit is 0 or +1 (s + C < 2 * 16^64): both occur, no other can"
        scalars[name] = {V.from_be_words(w) for _, w in op.sets}
        for s in [0, 1, R - 1, N, N - 1] + [int(c * 64, 16) for c in "078f"]:
            assert s in scalars[name], hex(s)
    both = scalars["recode_g1"] | scalars["recode_g2"]
    assert all(8 << (4 * p) in both for p in range(64)) and all(s in both for s in test_g2smul_model.SCALARS)
    seen = {(d < 0, abs(d)) for name in scalars for s in scalars[name] for d in g2smul_model.recode(s)}
    assert seen == {(False, a) for a in range(8)} | {(True, a) for a in range(1, 9)}          # every digit -8 .. 7
    for name, dw in (("select_g1", V.G1_DW), ("select_g2", V.G2_DW)):
        op = V.OPS[name]
        assert {(w[0], w[1]) for _, w in op.sets} == {(ad, k) for ad in range(9) for k in (0, M32)}
        for (cls, w), e in zip(op.sets, V.expected(name)):
            T = [tuple(w[2 + e_ * dw:2 + (e_ + 1) * dw]) for e_ in range(8)]
            assert len(set(T)) == 8, "entries all distinct"
            if w[0] and not w[1]:
                assert tuple(e) == T[w[0] - 1]
            if not w[0]:
                assert tuple(e) == (T[0] if w[1] else (0,) * dw)


def test_layout():
    """item i is the same set whatever n is; 257 items meet every set; a wavefront of inv_uni holds one value; the lanes of
    a wavefront of the long HMACs hold many lengths; zero sits next to non-zero values in inv"""
    for name, op in V.OPS.items():
        w257, i257, _, _ = V.call(name, 257)
        assert set(i257) == set(range(len(op.sets))), name
        for n in V.N_ITEMS[:-1]:
            w, idx, want, chk = V.call(name, n)
            assert idx == i257[:n] and len(w) == n * op.win and len(want) == len(chk) == n
            if not op.strided:
                assert w == w257[:len(w)]
    _, idx, _, _ = V.call("inv_uni", 257)
    assert all(len(set(idx[64 * k:64 * k + 64])) == 1 for k in range(4)) and len(set(idx)) == 5
    for name in ("hmac_long", "hmac_long_pair"):
        _, idx, _, _ = V.call(name, 257)
        for k in range(4):
            lens = {V.OPS[name].sets[s][1][0] for s in idx[64 * k:64 * k + 64]}
            assert len(lens) >= 10 and len({V.hdk_blocks(n) for n in lens}) >= 3, (name, k, sorted(lens))
    _, idx, _, _ = V.call("inv", 257)
    zero = [V.OPS["inv"].sets[k][0] == "zero" for k in idx]
    assert any(zero[i] != zero[i + 1] for i in range(63)) and any(zero[i] != zero[i + 1] for i in range(64, 255))
    # select_g2: dword d of item i's table at word 2 n + d n + i
    words, idx, _, _ = V.call("select_g2", 65)
    sets = V.OPS["select_g2"].sets
    assert all(words[2 * i:2 * i + 2] == sets[k][1][:2] for i, k in enumerate(idx))
    assert all(words[2 * 65 + d * 65 + i] == sets[k][1][2 + d] for i, k in enumerate(idx) for d in (0, 1, 41, 8 * V.G2_DW - 1))


def test_sets_lie_inside_their_preconditions():
    ops = V.OPS
    for name in ("add_mod_n", "add_mod_n_masked", "add", "add_masked", "sub", "sqr", "neg", "to_mont", "from_mont", "to_mont_masked",
                 "from_mont_masked", "inv", "inv_uni", "sd_cross_equal"):
        for cls, w in ops[name].sets:
            assert all(V.from_words(w[8 * i:8 * i + 8]) < N for i in range(len(w) // 8)), (name, cls)
    for name in ("mul", "mul_masked"):
        for cls, w in ops[name].sets:
            a, b = V.two(w)
            assert a < N and (N <= b < R if cls == "wide_b" else b < N), (name, cls)
        vals = {V.two(w) for _, w in ops[name].sets}
        for v in (0, 1, 2, N - 1, V.R1, V.R2, V.ALL1 ^ V.ALT) + tuple(V.POW32) + tuple(V.POW32M1[:7]):
            assert any(a == v for a, _ in vals) and any(b == v for _, b in vals), hex(v)
        assert {b for (a, b) in vals if b >= N} >= {N, N + 1, 2 * N - 1, 2 * N, 2 * N + 1, 1 << 255, R - 1}
    for name in ("sub_n_if_ge", "reduce_n", "sub_n_if_ge_masked", "reduce_n_masked"):
        vals = {V.from_words(w) for _, w in ops[name].sets}
        assert vals >= set(V.WIDE)
    for name in ("dot_term", "dot_term_masked"):
        for cls, w in ops[name].sets:
            assert V.from_be_words(w[:8]) < N                     # the coefficient: never a caller's bytes, always below n
        assert {V.from_be_words(w[8:]) for _, w in ops[name].sets} >= set(V.Y_EDGE)
    for cls, w in ops["sum_term_masked"].sets:
        assert V.from_words(w[8:]) < N
    for cls, w in ops["lagrange_weight"].sets:
        k, j = w[0], w[1]
        xs = [V.from_words(w[2 + 8 * i:10 + 8 * i]) for i in range(k)]
        assert k in (1, 2, 3, 67) and j < k and all(x < N for x in xs)
        zero = V.from_words(V.expected("lagrange_weight")[ops["lagrange_weight"].sets.index((cls, w))]) == 0
        assert zero == (cls in ("repeated", "zero_self")), cls
    assert {(w[0], w[1]) for _, w in ops["lagrange_weight"].sets} == {(k, j) for k in (1, 2, 3, 67) for j in (0, k // 2, k - 1)}
    for cls, w in ops["lagrange_point"].sets:
        x = V.from_be_words(w)
        assert (cls == "refused") == (x == 0 or x >= N)
    assert {"refused", "point"} == {c for c, _ in ops["lagrange_point"].sets}
    assert {w[0] for _, w in ops["lagrange_den"].sets} == {1, 2, 3, 67}
    for cls, w in ops["lagrange_den"].sets:
        assert all(V.from_words(w[1 + 8 * i:9 + 8 * i]) < N for i in range(w[0]))
    assert {w[0] for _, w in ops["poly_horner_masked"].sets} == {1, 2, 3, 16}
    for cls, w in ops["poly_horner_masked"].sets:
        assert all(V.from_words(w[1 + 8 * i:9 + 8 * i]) < N for i in range(w[0] + 1))
    for cls, w in ops["sd_neg_coord"].sets:
        assert int.from_bytes(V.words_bytes(w), "big") < V.Q
    iv = {V.from_words(w) for _, w in ops["inv"].sets}
    assert iv >= {0, 1, N - 1, 2, (N + 1) // 2, V.R1} | {c * R % N for c in (1, N - 1, 2, (N + 1) // 2, V.R1)}
    # sha: the lengths, fills and alignments asked for
    assert {w[0] for _, w in ops["hmac_key"].sets} >= {0, 1, 31, 32, 33, 64}
    assert {w[0] for _, w in ops["pad_hmac_block"].sets} >= {0, 1, 3, 4, 37, 53, 55} and max(w[0] for _, w in ops["pad_hmac_block"].sets) <= 55
    assert {w[0] for _, w in ops["child_hmacs"].sets} == {w[0] for _, w in ops["path_step"].sets} == {8, 12}
    hl = ops["hmac_long"].sets
    assert {(w[0], w[1]) for _, w in hl} == {(n, s) for n in V.LONG_LENS for s in (M32, 0, 1)}
    assert {(w[0], w[2]) for _, w in hl} >= {(n, sh) for n in V.LONG_LENS[1:] for sh in range(3)} and {c for c, _ in hl} == {"zeros", "ones", "random"}
    assert {(w[0], w[1]) for _, w in ops["hmac_long_pair"].sets} == {(n, sh) for n in V.LONG_LENS for sh in range(4)}
    for name, hdr in (("hmac_long", 19), ("hmac_long_pair", 18), ("long_word", 5)):
        for _, w in ops[name].sets:
            assert w[0] + 3 <= 4 * V.MSGW
    assert {w[0] for _, w in ops["hpk_digest"].sets} >= {1, 2, 3, 4, 5, 8, 9} and max(w[0] for _, w in ops["hpk_digest"].sets) <= V.MAXKEYS
    for cls, idx in V.EXP_INDEX.items():
        lo = {"below_n": 0, "n_to_2n": N, "above_2n": 2 * N}[cls]
        for i in idx:
            assert lo <= V.exp_value(V.EXP_DIGEST, i) < min(lo + N, R), (cls, i)


def test_sets_found_by_emulation_have_their_property():
    """cios() is frs::mul word for word; it equals the integer Montgomery product on every product set, and the properties
    the docstring of fr_vectors.py assigns to sets are there"""
    for name in ("mul", "mul_masked"):
        fired, t8_at, t8_zero, m_seen, results, exact_n = set(), set(), False, set(), set(), False
        for cls, w in V.OPS[name].sets:
            a, b = V.two(w)
            r, ms, t8s, f = V.cios(a, b)
            assert r == V.mont(a, b) == (V.pre_sub(a, b) - (N if f else 0)) and f == (V.pre_sub(a, b) >= N), (cls, hex(a), hex(b))
            assert V.pre_sub(a, b) < a + N                    # the bound of the check file's header: t < a + n
            if cls in ("fires", "stays"):
                assert f == (cls == "fires") and r in (1, 2, N - 1, N - 2)
            if cls != "wide_b":
                assert V.pre_sub(a, b) != N                   # unreachable below n
                fired.add(f)
                results.add(r)
            exact_n |= V.pre_sub(a, b) == N
            t8_at |= {i for i, t in enumerate(t8s) if t}
            t8_zero |= not any(t8s) and a != 0 and b != 0
            m_seen |= set(ms)
        assert fired == {True, False} and t8_at == set(range(8)) and t8_zero and {0, M32} <= m_seen and {0, N - 1, 1} <= results and exact_n
        seen = {(V.mont(*V.two(w)), V.cios(*V.two(w))[3]) for c, w in V.OPS[name].sets if c != "wide_b"}
        assert seen >= {(1, True), (1, False), (2, True), (2, False), (N - 1, False), (N - 2, False)}    # ((2^128, 2^128) is an `edge` pair)


def test_python_compression_against_hashlib():
    """sha_compress, key_states and hmac_from_states (the references where a chaining state is an operand) against hashlib / hmac"""
    rnd = V._rnd("model")
    for n in list(range(0, 130)) + [200, 1000]:
        msg = bytes(rnd.randrange(256) for _ in range(n))
        assert V.be_state(V.sha_blocks(V.IV, V.padded(msg, 0))) == hashlib.sha256(msg).digest()
        for klen in (0, 1, 11, 20, 32, 64):
            key = bytes(rnd.randrange(256) for _ in range(klen))
            assert V.hmac_from_states(V.key_states(key), msg) == V.hmac_words(key, msg)
        assert V.hdk_blocks(n) == len(V.padded(msg, 64)) // 64 and V.hdk_blocks(n, True) == len(V.padded(msg + b"\1", 64)) // 64
    for name in ("hmac_long", "hmac_long_pair"):              # the long forms once more, from the hmac module and the bytes
        key = b"BLS private key seed" if name == "hmac_long" else b"BLS HD seed"
        for (cls, w), e in zip(V.OPS[name].sets, V.expected(name)):
            if name == "hmac_long":
                msg = V.long_message(w, 19, w[0], w[2])
                assert e == V.hmac_words(key, msg + (b"" if w[1] == M32 else bytes([w[1]])))
            else:
                msg = V.long_message(w, 18, w[0], w[1])
                assert e == V.hmac_words(key, msg + b"\0") + V.hmac_words(key, msg + b"\1")
            assert {"zeros": set(msg) <= {0}, "ones": set(msg) <= {255}, "random": True}[cls]


# ---- (c) mutants -------------------------------------------------------------------------------------------------------
def _w8(f):
    return lambda w: V.words8(f(*[V.from_words(w[8 * i:8 * i + 8]) for i in range(len(w) // 8)]) % R)


def _sub_gt(x):
    return x - N if x > N else x


def _long_mut(hdr, suffixes, extra=False, swap=False):
    def ref(w):
        n, shift = w[0], w[hdr - 17]
        out = []
        for sfx in suffixes(w):
            m = V.long_message(w, hdr, n, shift)
            if sfx is not None:
                m = (m[:-1] + bytes([sfx]) + m[-1:]) if swap and m else m + bytes([sfx])
            out += V.hmac_from_states(w[hdr - 16:hdr], m, 1 if extra and len(m) % 64 == 55 else 0)
        return out
    return ref


_one = lambda w: [None if w[1] == M32 else w[1]]
_pair = lambda w: [0, 1]


def _recode_no_ninth(w):
    from vmgen import g2smul_model
    t = (V.from_be_words(w) + g2smul_model.BIAS) % R
    return V.digit_words([((t >> (4 * i)) & 15) - 8 for i in range(V.DIGITS)])


def _select_no_keep0(dw):
    return lambda w: w[2 + (w[0] - 1) * dw:2 + w[0] * dw] if w[0] else [0] * dw


def _neg_coord_mut(ws):
    y = int.from_bytes(V.words_bytes(ws), "big")
    return V.bytes_words((V.Q - y).to_bytes(48, "big"))


def _long_word_swapped(w):
    n, has, suffix, off, shift = w[:5]
    m = V.long_message(w, 5, n, shift)
    stream = ((m[:-1] + bytes([suffix]) + m[-1:]) if has and m else m + (bytes([suffix]) if has else b"")) + b"\x80"
    return V.state_words((stream + b"\0" * (off + 4))[off:off + 4])


def _quot_inv_is_one(w):
    a0, b0 = V.from_be_words(w[:8]) % N, V.from_be_words(w[8:]) % N
    q = a0 if b0 else 0
    return V.be_words((N - q) % N) + [int(q == 1)]


MUTANTS = {
    "the last subtraction on > instead of >=": {
        "sub_n_if_ge": _w8(_sub_gt), "sub_n_if_ge_masked": _w8(_sub_gt), "reduce_n": _w8(lambda x: _sub_gt(_sub_gt(x))),
        "reduce_n_masked": _w8(lambda x: _sub_gt(_sub_gt(x))), "add_mod_n": _w8(lambda a, b: _sub_gt(a + b)), "add": _w8(lambda a, b: _sub_gt(a + b)),
        "mul": _w8(lambda a, b: V.cios(a, b, ge=False)[0]), "mul_masked": _w8(lambda a, b: V.cios(a, b, ge=False)[0])},
    "t[8] dropped": {"mul": _w8(lambda a, b: V.cios(a, b, drop_t8=True)[0]), "mul_masked": _w8(lambda a, b: V.cios(a, b, drop_t8=True)[0]),
                     "sqr": _w8(lambda a: V.cios(a, a, drop_t8=True)[0]), "to_mont": _w8(lambda a: V.cios(a, V.R2, drop_t8=True)[0])},
    "m from t[1]": {"mul": _w8(lambda a, b: V.cios(a, b, m_from=1)[0]), "sqr": _w8(lambda a: V.cios(a, a, m_from=1)[0]),
                    "from_mont": _w8(lambda a: V.cios(a, 1, m_from=1)[0])},
    "reduce_n with one subtraction": {
        "reduce_n": _w8(lambda x: x - N if x >= N else x), "reduce_n_masked": _w8(lambda x: x - N if x >= N else x),
        "hpk_exponent": lambda w: V.words8((lambda v: v - N if v >= N else v)(V.exp_value(V.be_state(w[1:]), w[0]))),
        "sum_term_masked": lambda w: V.words8((lambda s: s - N if s >= N else s)((lambda v: v - N if v >= N else v)(V.from_be_words(w[:8])) + V.from_words(w[8:])))},
    "inv with exponent n - 1": {"inv": _w8(lambda x: V.R1 if x else 0), "inv_uni": _w8(lambda x: V.R1 if x else 0), "quotient_scalar": _quot_inv_is_one,
                                "lagrange_den": lambda w: V.words8(V.R1 if sum(V.from_words(w[1 + 8 * i:9 + 8 * i]) for i in range(w[0])) % N else 0)},
    "neg(0) = n": {"neg": _w8(lambda x: N - x)},
    "padding off by one block at 55 / 56": {"long_blocks": lambda w: [(w[0] + (0 if w[1] == M32 else 1) + 9) // 64 + 1],
                                            "hmac_long": _long_mut(19, _one, extra=True), "hmac_long_pair": _long_mut(18, _pair, extra=True)},
    "the suffix byte before the last message byte": {"hmac_long": _long_mut(19, _one, swap=True), "hmac_long_pair": _long_mut(18, _pair, swap=True),
                                                     "long_word": _long_word_swapped},
    "hpk::digest with an extra padding block at k mod 4 = 0": {
        "hpk_digest": lambda w: V.sha_blocks(V.IV, V.padded(V.words_bytes(w[4:4 + 12 * w[0]]), 0, 1 if w[0] % 4 == 0 else 0))},
    "digits from s + C without the ninth word": {"recode_g1": _recode_no_ninth, "recode_g2": _recode_no_ninth},
    "select_entry ignoring keep0": {"select_g1": _select_no_keep0(V.G1_DW), "select_g2": _select_no_keep0(V.G2_DW)},
    "neg_coord mapping 0 to q": {"sd_neg_coord": _neg_coord_mut, "sd_neg_point": lambda w: w[:24] + _neg_coord_mut(w[24:36]) + _neg_coord_mut(w[36:48])},
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_every_mutant_is_caught_by_every_op_it_belongs_to(mutant):
    assert len(MUTANTS) >= 10
    for name, mref in MUTANTS[mutant].items():
        op = V.OPS[name]
        want = V.expected(name)
        caught = [k for k, (_, w) in enumerate(op.sets) if [int(v) & M32 for v in mref(w)] != want[k]]
        assert caught, "%s: no set of %s tells the mutant from the reference" % (mutant, name)
