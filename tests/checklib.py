"""The Python side the nine check-library GPU tests share (test_gpu_fp28, test_gpu_fq32, test_gpu_wide, test_gpu_ml_steps,
test_gpu_fr, test_gpu_curve, test_gpu_fx, test_gpu_vm, test_gpu_h2c_check): loading a library, one call with its return-code message, the per-lane comparison loop of the
lane-layout libraries and the per-set comparison loop of wide, ml, curve and fx (test_gpu_vm uploads whole programs and has its own
loop over teams, test_gpu_h2c_check its own loop over more sets than one call holds).  The return codes are csrc/check_runner.h's."""
import ctypes
import os

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "python-bls_amd", "csrc")


def load(stem, symbol):
    """the exported function `symbol` of csrc/<stem>.so; both buffers are c_void_p: a ctypes array or an address"""
    import torch  # noqa: F401  (first, as bls_py._native.load_library: both bind to one HIP runtime)
    path = os.path.join(CSRC, stem + ".so")
    assert os.path.exists(path), "%s.so is not built: run __graft_entry__.build() (make -C python-bls_amd/csrc)" % stem
    fn = getattr(ctypes.CDLL(path), symbol)
    fn.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]
    fn.restype = ctypes.c_int
    return fn


def call(lib_fn, op, words, n, dtype):
    """one call of n items: the output words of every item"""
    cin = np.array(words, dtype=dtype)
    cout = np.zeros(n * op.wout, dtype=dtype)
    rc = lib_fn(op.code, cin.ctypes.data, cin.size, n, cout.ctypes.data, cout.size)
    assert rc == 0, ("%s, %d items: %s returned %d (-3: a guard record was written; -4: a record refused before the launch; > 0: HIP error)"
                     % (op.name, n, lib_fn.__name__, rc))
    got = cout.tolist()
    return [got[i * op.wout:(i + 1) * op.wout] for i in range(n)]


def run_group(lib_fn, V, group, dtype=np.uint32, item_call=None):
    """every op of a group of a lane-layout vectors module, with every count of V.N_ITEMS: each item against its expected words
    and, once per set at the largest count (every item for an op.wave op), the independent check on the device's own words.
    item_call(name, n) gives (input words, set of each item, expected words of each item, check of each item or None)."""
    item_call = item_call or V.call
    ran = 0
    for op in V.OPS.values():
        if op.group != group:
            continue
        for n in V.N_ITEMS:
            words, idx, want, chk = item_call(op.name, n)
            got = call(lib_fn, op, words, n, dtype)
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
                if n == V.N_ITEMS[-1] and c is not None and (getattr(op, "wave", False) or k not in checked):
                    checked.add(k)
                    c(g)
            if n == V.N_ITEMS[-1]:
                assert set(idx) == set(range(len(op.sets))), op.name
            ran += 1
    assert ran and ran % len(V.N_ITEMS) == 0


def run_sets(lib_fn, V, op, counts, checks=False):
    """an op of a per-set vectors module (wide, ml, curve) with every count, then further calls of the largest count until every set
    has run; every output word is compared exactly, except where the expected word is None (wide's write sink).  checks: a set's
    fifth entry is its independent check (or None), run on the device's own words once per set; where device and model differ it
    says which of them is wrong"""
    checked = set()

    def one(sets):
        n = len(sets)
        got = call(lib_fn, op, [w for k in sets for w in op.sets[k][1]], n, np.int32)
        for i, k in enumerate(sets):
            tag, want = op.sets[k][0], op.sets[k][2]
            chk = op.sets[k][4] if checks else None
            if got[i] == want:
                if chk is not None and k not in checked:
                    checked.add(k)
                    chk(got[i])
                continue
            if chk is not None:                       # who is wrong: the independent check on the device's words decides
                try:
                    chk(got[i])
                except AssertionError as err:
                    raise AssertionError("%s, %d items, item %d, set %s: the device is wrong (%s)" % (op.name, n, i, tag, err))
            bad = [(j, got[i][j], w) for j, w in enumerate(want) if w is not None and got[i][j] != w]
            assert not bad, "%s, %d items, item %d, set %s: %d words differ, first (word, got, want) %s" % (op.name, n, i, tag, len(bad), bad[:4])
        return set(sets)

    seen = set()
    for n in counts:
        seen |= one(V.call_sets(op, n))
    base = counts[-1]
    while len(seen) < len(op.sets):                # the sets a call of the largest count has not reached yet
        assert base < 64 * counts[-1], op.name
        seen |= one(V.call_sets(op, counts[-1], base))
        base += counts[-1]
