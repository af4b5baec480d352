"""GPU: run_rounds, the round interpreter under every wavefront-VM kernel (csrc/blsgpu_kernels.hip), on uploaded programs and
scratchpad images through the test-only library csrc/blsgpu_vm_check.hip (libblsgpu_vmcheck.so), in the three geometries production
uses (one, four and eight teams per workgroup).  Programs, the word machine and the references are tests/vm_vectors.py's;
tests/test_vm_vectors_model.py checks them on the CPU.  No tolerances: every word of every slot of every returned image equals the
word machine's, and every slot read as an integer mod q equals vmgen/tablesim.py's (the independent reference, on the device's own
words); return value, functor calls and stash words likewise.  The production tables run from a seeded image, cut at every segment
boundary of every script: tools/trace_rounds.py as an assertion."""
import numpy as np
import pytest

import checklib
import vm_vectors as V

pytestmark = pytest.mark.gpu
Q = V.Q


@pytest.fixture(scope="module")
def lib():
    return checklib.load("libblsgpu_vmcheck", "blsgpu_vm_check")


def _raw(lib, code, words, n, nout):
    w, o = np.asarray(words, dtype=np.uint32), np.zeros(nout, dtype=np.uint32)
    return lib(code, w.ctypes.data, w.size, n, o.ctypes.data, o.size), o


def _img_words(imgs):
    return np.frombuffer(b"".join(v.to_bytes(48, "little") for img in imgs for v in img), dtype=np.uint32)


def _ints(words, nslots):
    b = words.tobytes()
    return [int.from_bytes(b[48 * s:48 * s + 48], "little") for s in range(nslots)]


def _run(lib, op, rounds, table_words, ntable, nslots, imgs, tpw, check_at=0, chk_slot=0):
    """one call: ([image words of every team], [(ret, calls, stash words)])"""
    n = len(imgs)
    hdr = np.array([len(rounds), nslots, ntable, check_at, chk_slot, tpw, 0, 0] + [x for r in rounds for x in r], dtype=np.uint32)
    words = np.concatenate([hdr, table_words, _img_words(imgs)])
    nout = n * (nslots * 12 + V.TRAILER)
    rc, out = _raw(lib, V.OPS[op], words, n, nout)
    assert rc == 0, "%s, %d teams of %d a workgroup: returned %d (-3: a guard record was written; -4: refused; > 0: HIP error)" % (op, n, tpw, rc)
    tr = out[n * nslots * 12:].reshape(n, V.TRAILER)
    return [out[t * nslots * 12:(t + 1) * nslots * 12] for t in range(n)], [(int(r[0]), int(r[1]), r[2:].tolist()) for r in tr]


def _table_words(table):
    t = np.array(list(table) + [0] * (len(table) & 1), dtype=np.uint32)
    return t[0::2] | (t[1::2] << 16)


_EXPECTED = {}


def _expected(p, op):
    """per image of a program: (the word machine's image and trailer, tablesim's residues, stash residues, ret, calls) -- once"""
    if (p.name, op) not in _EXPECTED:
        m = V.WordMachine(p.table(), p.images)
        check_at, slot = p.check if p.check else (0, 0)
        res = m.run(p.rounds, op, check_at, slot)
        _EXPECTED[(p.name, op)] = [(m.teams[k], res[k], V.reference(p, op, p.images[k])) for k in range(p.nimg)]
    return _EXPECTED[(p.name, op)]


def _check_class(lib, cls):
    ran = 0
    for p in V.programs():
        if p.cls != cls:
            continue
        tw = _table_words(p.table())
        check_at, slot = p.check if p.check else (0, 0)
        for op in p.ops:
            exp = _expected(p, op)
            for tpw in V.geometries(p):
                imgs = [p.images[t % p.nimg] for t in range(8)]
                got, trailers = _run(lib, op, p.rounds, tw, len(p.table()), p.nslots, imgs, tpw, check_at, slot)
                for t in range(8):
                    where = "%s under %s, %d teams a workgroup, team %d" % (p.name, op, tpw, t)
                    words, (ret, calls, sw), (res, stash, rret, rcalls) = exp[t % p.nimg]
                    mine = _ints(got[t], p.nslots)
                    # the independent reference first: tablesim on the device's own words decides who is wrong
                    bad = [s for s in range(p.nslots) if mine[s] % Q != res[s]]
                    assert not bad, "%s: slots %s differ from tablesim: the device is wrong" % (where, bad[:8])
                    assert all(v < 2 * Q for v in mine), where + ": a slot is not below 2q"
                    assert trailers[t][:2] == (rret, rcalls), "%s: (return value, functor calls) %s, tablesim's run says %s" % (where, trailers[t][:2], (rret, rcalls))
                    bad = [s for s in range(p.nslots) if mine[s] != words[s]]
                    assert not bad, "%s: slots %s have tablesim's residue and not the word machine's words" % (where, bad[:8])
                    assert trailers[t] == (ret, calls, sw), where + ": trailer"
                    if stash is not None:
                        assert [V.F32.from_words(trailers[t][2][12 * k:12 * k + 12]) % Q for k in range(12)] == stash, where + ": stash"
                    if p.cls == "teams":                 # the last twelve slots are referenced by no round
                        assert mine[-12:] == imgs[t][-12:], where
                ran += 1
    assert ran
    return ran


@pytest.mark.parametrize("cls", V.CLASSES)
def test_program_class(lib, cls):
    """every op of every program of the class in every geometry it fits, eight teams a call, each team against its own image's run"""
    _check_class(lib, cls)


def test_light_without_stash_is_the_program_without_its_windows(lib):
    """stash = nullptr: the same program leaves the image as a program without those rounds leaves it -- both on the device"""
    for p in V.programs():
        if p.cls != "stash":
            continue
        tw = _table_words(p.table())
        a, _ = _run(lib, "RUN_LIGHT", p.rounds, tw, len(p.table()), p.nslots, p.images[:1], 1)
        b, _ = _run(lib, "RUN_LIGHT", V.strip_windows(p.rounds), tw, len(p.table()), p.nslots, p.images[:1], 1)
        assert (a[0] == b[0]).all(), p.name


def test_production_tables_at_every_segment_boundary(lib):
    """every flat program of emit.build_tables() under the mode its kernels use, cut at every segment boundary of its script, the stage
    segments and the directly called segments: every slot against the word machine and tablesim, snapshotted in one CPU pass"""
    progs, data, consts = V.production()
    tw = _table_words(data)
    for name, op, rounds, cuts in progs:
        img = V.production_image(name, op, rounds, data, consts)
        snaps = V.production_snapshots(op, rounds, cuts, data, img)
        for c in cuts:
            got, trailers = _run(lib, op, rounds[:c], tw, len(data), len(img), [img], 1)
            words, sw, res = snaps[c]
            mine = _ints(got[0], len(img))
            bad = [s for s in range(len(img)) if mine[s] % Q != res[s]]
            assert not bad, "%s cut at round %d: slots %s differ from tablesim: the device is wrong" % (name, c, bad[:8])
            bad = [s for s in range(len(img)) if mine[s] != words[s]]
            assert not bad, "%s cut at round %d: slots %s have the residue and not the word machine's words" % (name, c, bad[:8])
            assert trailers[0] == (1, 0, sw), (name, c)


def test_bad_tables_are_refused_before_the_launch(lib):
    """every refusal of csrc/vm_check_plan.h returns -4 (sizes -2, an unknown op -1) and launches nothing; the decisions themselves are
    covered on the CPU by tests/test_vm_check_host.py, which shares REFUSALS"""
    import vm_refusals as RF
    for name, op, words, n, nout, want in RF.cases():
        rc, out = _raw(lib, op, words, n, nout)
        assert rc == want, (name, rc, want)
        assert rc == 0 or not out.any(), name + ": output written"
