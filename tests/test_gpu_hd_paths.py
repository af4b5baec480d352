"""HD path derivation on the GPU (blsgpu_hd_paths, csrc/blsgpu_g1fix.hip): the records of tests/golden/hd_paths.json
(generated from the reference) through the real engine in both modes and both forms, agreement with the single-level
entry blsgpu_hd_children (depth 1 byte for byte, random deeper paths, a 256 x 256 grid and 65 536 paths of depth 3 by
digest), and every refusal with untouched outputs."""
import ctypes
import hashlib
import random

import pytest

from hd_paths_vectors import check_digest, check_grid_record, check_private_record, check_public_record

pytestmark = pytest.mark.gpu

H31 = 2**31
WIDTHS = (32, 32, 96, 48, 4)            # chain code, key, affine, serialised, parent fingerprint


@pytest.fixture
def hip_backend(engine):
    from bls_py import backend
    old = backend._provider
    backend.use(backend.HipProvider())
    yield
    backend.use(old)


@pytest.fixture(scope="module")
def fx(golden):
    return golden("hd_paths.json")


def _aff(pk):
    from bls_py import hostmath as H
    return H.g1_affine_bytes(H.jac_to_affine(H.F1, pk.value._jac()))


def _record(k):
    """the 160-byte parent record of an extended key"""
    sk = getattr(k, "private_key", None)
    pk = sk.get_public_key() if sk is not None else k.public_key
    return k.chain_code + _aff(pk) + (sk.serialize() if sk is not None else bytes(32))


def _keys(seed=b"gpu paths"):
    from bls_py.keys import ExtendedPrivateKey
    esk = ExtendedPrivateKey.from_seed(seed)
    return esk, esk.get_extended_public_key()


def test_fixture_through_the_engine(fx, hip_backend):
    for rec in fx["private"]:
        check_private_record(rec, full=True)
    check_public_record(fx["public"], full=True)
    check_grid_record(fx["grid"], full=True)


def _dev_call(e, records, priv, parent_of, paths, fill=None, outs=None):
    """blsgpu_hd_paths_dev over torch buffers -> the five outputs as bytes (key: None in public mode)"""
    import torch
    dev = torch.device("cuda", 0)
    n, depth = len(paths), len(paths[0])
    d_par = torch.tensor(list(records), dtype=torch.uint8, device=dev)
    d_of = torch.tensor(parent_of, dtype=torch.int64, device=dev).to(torch.int32) if parent_of is not None else None
    d_idx = torch.tensor([i for p in paths for i in p], dtype=torch.int64, device=dev).to(torch.int32)
    if outs is None:
        outs = [torch.full((w * n,), 0xAA, dtype=torch.uint8, device=dev) for w in WIDTHS]
    st = torch.cuda.current_stream(dev)
    try:
        e.hd_paths_dev(d_par.data_ptr(), len(records) // 160, priv, d_of.data_ptr() if d_of is not None else None, d_idx.data_ptr(), depth, n,
                       outs[0].data_ptr(), outs[1].data_ptr() if priv else None, outs[2].data_ptr(), outs[3].data_ptr(), outs[4].data_ptr(),
                       st.cuda_stream)
    finally:
        st.synchronize()
    got = [bytes(o.cpu().numpy()) for o in outs]
    if not priv:
        assert got[1] == b"\xaa" * len(got[1])              # out_sk is ignored in public mode
        got[1] = None
    return tuple(got)


def test_fixture_through_the_dev_form(fx, engine):
    from bls_py.keys import ExtendedPrivateKey, ExtendedPublicKey
    rec = fx["private"][0]
    esk = ExtendedPrivateKey.from_seed(bytes.fromhex(rec["seed"]))
    sers = [None] * len(rec["paths"])
    for depth in range(1, 7):
        pos = [j for j, p in enumerate(rec["paths"]) if len(p) == depth]
        paths = [rec["paths"][j] for j in pos]
        host = engine.hd_paths(_record(esk), True, None, paths)
        assert _dev_call(engine, _record(esk), True, None, paths) == host
        for t, j in enumerate(pos):
            sers[j] = (bytes([0, 0, 0, 1, depth]) + host[4][4 * t:4 * t + 4] + paths[t][-1].to_bytes(4, "big") + host[0][32 * t:32 * t + 32] +
                       host[1][32 * t:32 * t + 32])
    check_digest(sers, rec["esk"])
    rec = fx["public"]
    xpub = ExtendedPublicKey.from_bytes(bytes.fromhex(rec["xpub"]))
    sers = [None] * len(rec["paths"])
    for depth in range(1, 7):
        pos = [j for j, p in enumerate(rec["paths"]) if len(p) == depth]
        paths = [rec["paths"][j] for j in pos]
        host = engine.hd_paths(_record(xpub), False, [0] * len(pos), paths)
        assert _dev_call(engine, _record(xpub), False, [0] * len(pos), paths) == host
        for t, j in enumerate(pos):
            sers[j] = (bytes([0, 0, 0, 1, xpub.depth + depth]) + host[4][4 * t:4 * t + 4] + paths[t][-1].to_bytes(4, "big") +
                       host[0][32 * t:32 * t + 32] + host[3][48 * t:48 * t + 48])
    check_digest(sers, rec["epk"])


def test_depth_one_equals_hd_children(engine, hip_backend):
    rnd = random.Random(31)
    esk, _ = _keys()
    parents = esk.private_child_batch([H31 + 1, 5, H31 + 9, 0])
    for priv in (True, False):
        keys = parents if priv else [k.get_extended_public_key() for k in parents]
        records = b"".join(_record(k) for k in keys)
        idx = [[rnd.randrange(2**32 if priv else H31) for _ in range(300)] for _ in keys]
        parent_of = [a for a in range(len(keys)) for _ in range(300)]
        rnd.shuffle(parent_of)
        slot = [0] * len(keys)
        paths = []
        for a in parent_of:
            paths.append([idx[a][slot[a]]])
            slot[a] += 1
        got = engine.hd_paths(records, priv, parent_of, paths)
        single = []
        for a, k in enumerate(keys):
            pk = k.private_key.get_public_key() if priv else k.public_key
            single.append(engine.hd_children(k.chain_code, _aff(pk), k.private_key.serialize() if priv else None, idx[a]) +
                          (pk.get_fingerprint().to_bytes(4, "big") * 300,))
        slot = [0] * len(keys)
        for j, a in enumerate(parent_of):
            t = slot[a]
            slot[a] += 1
            for o, w in enumerate(WIDTHS):
                if got[o] is None:
                    assert single[a][o] is None and not priv
                    continue
                assert got[o][w * j:w * (j + 1)] == single[a][o][w * t:w * (t + 1)], (priv, j, a, o)
    # one output form at a time, and without the fingerprint
    rec = _record(parents[0])
    full = engine.hd_paths(rec, True, None, [[1], [H31]])
    assert engine.hd_paths(rec, True, None, [[1], [H31]], ser=False, fp=False) == (full[0], full[1], full[2], None, None)
    assert engine.hd_paths(rec, True, None, [[1], [H31]], aff=False) == (full[0], full[1], None, full[3], full[4])


def test_random_paths_equal_folded_children(engine, hip_backend):
    from bls_py.keys import ExtendedPrivateKey, ExtendedPublicKey
    rnd = random.Random(32)
    esk, epk = _keys(b"fold")
    for depth in range(2, 9):
        paths = [[rnd.randrange(2**32) for _ in range(depth)] for _ in range(6)] + [[H31 + 1] * depth, [1] * depth]
        got = esk.private_path_batch(paths)
        for k, p in zip(got, paths):
            want = esk
            for i in p:
                want = want.private_child(i)
            assert k.serialize() == want.serialize(), p
            assert k.get_extended_public_key().serialize() == want.get_extended_public_key().serialize(), p
        soft = [[rnd.randrange(H31) for _ in range(depth)] for _ in range(6)]
        for k, p in zip(epk.public_path_batch(soft), soft):
            want = epk
            for i in p:
                want = want.public_child(i)
            assert k.serialize() == want.serialize(), p
        assert esk.public_path_batch(soft) == epk.public_path_batch(soft)
    # a key at infinity as parent: what the single-level entry does with it, level by level
    inf = bytes(32) + bytes(96) + bytes(32)
    got = engine.hd_paths(inf, False, None, [[3, 4]])
    c1, _, a1, _ = engine.hd_children(bytes(32), bytes(96), None, [3])
    c2, _, a2, s2 = engine.hd_children(c1, a1, None, [4])
    assert got[0] == c2 and got[2] == a2 and got[3] == s2 and got[4] == hashlib.sha256(engine.hd_children(bytes(32), bytes(96), None, [3])[3]).digest()[:4]
    gotp = engine.hd_paths(inf, True, None, [[H31, 4]])                      # private key 0: public key at infinity
    c1, k1, a1, _ = engine.hd_children(bytes(32), bytes(96), bytes(32), [H31])
    c2, k2, a2, s2 = engine.hd_children(c1, a1, k1, [4])
    assert gotp[:4] == (c2, k2, a2, s2)


def _digest(outs):
    return [hashlib.sha256(o).hexdigest() if o is not None else None for o in outs]


def test_grid_256_by_256_against_per_parent_calls(engine):
    _, epk = _keys(b"grid")
    chain, _, aff, ser = engine.hd_children(epk.chain_code, _aff(epk.public_key), None, list(range(256)))
    records = b"".join(chain[32 * a:32 * a + 32] + aff[96 * a:96 * a + 96] + bytes(32) for a in range(256))
    parent_of = [a for a in range(256) for _ in range(256)]
    got = engine.hd_paths(records, False, parent_of, [[i] for _ in range(256) for i in range(256)])
    want = [[], [], [], []]
    for a in range(256):
        c, _, f, s = engine.hd_children(chain[32 * a:32 * a + 32], aff[96 * a:96 * a + 96], None, list(range(256)))
        fp = hashlib.sha256(ser[48 * a:48 * a + 48]).digest()[:4]
        for o, v in zip(want, (c, f, s, fp * 256)):
            o.append(v)
    assert _digest([got[0], got[2], got[3], got[4]]) == _digest([b"".join(o) for o in want])
    # and from the root as paths of depth 2, through the dev form
    two = _dev_call(engine, _record(epk), False, None, [[a, i] for a in range(256) for i in range(256)])
    assert _digest(two) == _digest(got)


def test_65536_paths_of_depth_3_against_level_by_level_calls(engine):
    """private mode, hardened / not / hardened: level 1 has 16 distinct indices, level 2 has 16 per level-1 key, level 3
    has 256 per level-2 key -- 1 + 16 + 256 blsgpu_hd_children calls on the same device give the same leaves"""
    rnd = random.Random(33)
    esk, _ = _keys(b"deep")
    l1 = [H31 + rnd.randrange(H31) for _ in range(16)]
    l2 = [[rnd.randrange(H31) for _ in range(16)] for _ in range(16)]
    l3 = [[[rnd.randrange(2**32) for _ in range(256)] for _ in range(16)] for _ in range(16)]
    paths = [[l1[a], l2[a][b], l3[a][b][c]] for a in range(16) for b in range(16) for c in range(256)]
    got = engine.hd_paths(_record(esk), True, None, paths)
    want = [[], [], [], [], []]
    c1, k1, a1, s1 = engine.hd_children(esk.chain_code, _aff(esk.private_key.get_public_key()), esk.private_key.serialize(), l1)
    for a in range(16):
        c2, k2, a2, s2 = engine.hd_children(c1[32 * a:32 * a + 32], a1[96 * a:96 * a + 96], k1[32 * a:32 * a + 32], l2[a])
        for b in range(16):
            leaf = engine.hd_children(c2[32 * b:32 * b + 32], a2[96 * b:96 * b + 96], k2[32 * b:32 * b + 32], l3[a][b])
            for o, v in zip(want, leaf + (hashlib.sha256(s2[48 * b:48 * b + 48]).digest()[:4] * 256,)):
                o.append(v)
    assert _digest(got) == _digest([b"".join(o) for o in want])
    order = list(range(65536))
    rnd.shuffle(order)                                       # lanes of one wavefront on unrelated paths
    shuffled = _dev_call(engine, _record(esk), True, None, [paths[j] for j in order])
    for o, w in enumerate(WIDTHS):
        assert hashlib.sha256(b"".join(shuffled[o][w * t:w * (t + 1)] for t in sorted(range(65536), key=order.__getitem__))).hexdigest() == \
            _digest(got)[o]


def _host_call(L, h, parents, n_parents, priv, parent_of, indices, depth, n, bufs):
    idx = (ctypes.c_uint32 * max(1, len(indices)))(*indices) if indices is not None else None
    pof = (ctypes.c_uint32 * max(1, len(parent_of)))(*parent_of) if parent_of is not None else None
    return L.blsgpu_hd_paths(h, parents, n_parents, priv, pof, idx, depth, n, *bufs)


def test_refusals_leave_outputs_untouched(engine):
    import torch
    from bls_py import _native
    L = _native.load_library()
    esk, epk = _keys()
    rec = _record(esk)
    n = 100

    def fresh():
        return [ctypes.create_string_buffer(b"\xaa" * (w * n), w * n) for w in WIDTHS]

    def untouched(bufs):
        return all(b is None or b.raw == b"\xaa" * len(b.raw) for b in bufs)

    soft = [1] * (2 * n)
    cases = [
        ("depth 0", (rec, 1, 1, None, soft, 0, n), "depth"),
        ("depth 256", (rec, 1, 1, None, [1] * (256 * n), 256, n), "depth"),
        ("no parents", (rec, 0, 1, None, soft, 2, n), "parent"),
        ("NULL parents", (None, 1, 1, None, soft, 2, n), "NULL"),
        ("NULL indices", (rec, 1, 1, None, None, 2, n), "NULL"),
        ("parent_of out of range", (rec * 2, 2, 1, [0] * 99 + [2], soft, 2, n), "parent index"),
        ("hardened, level 1", (rec, 1, 0, None, [1] * 99 + [H31] + [1] * n, 2, n), "Cannot derive hardened children from public key"),
        ("hardened, level 2", (rec, 1, 0, [0] * n, [1] * (2 * n - 1) + [2**32 - 1], 2, n), "Cannot derive hardened children from public key"),
    ]
    for name, args, text in cases:
        bufs = fresh()
        assert _host_call(L, engine.h, *args, bufs) == -22, name
        assert text in L.blsgpu_last_error().decode(), name
        assert untouched(bufs), name
    for name, drop, priv in (("no out_chain", 0, 1), ("no out_sk", 1, 1), ("no key output", (2, 3), 1), ("no key output", (2, 3), 0)):
        bufs = fresh()
        for d in (drop if isinstance(drop, tuple) else (drop,)):
            bufs[d] = None
        assert _host_call(L, engine.h, rec, 1, priv, None, soft, 2, n, bufs) == -22, name
        assert untouched(bufs), name
    # n == 0 writes nothing and succeeds; public mode ignores out_sk
    bufs = fresh()
    assert _host_call(L, engine.h, rec, 1, 1, None, soft, 2, 0, bufs) == 0 and untouched(bufs)
    assert _host_call(L, engine.h, rec, 1, 0, None, soft, 2, n, bufs) == 0
    assert bufs[1].raw == b"\xaa" * (32 * n) and not any(untouched([b]) for b in bufs[:1] + bufs[2:])
    with pytest.raises(_native.BlsGpuError):
        engine.hd_paths(_record(epk), False, None, [[0, H31 + 1]])
    # the dev form: the same refusals from the device scan, before anything is written
    dev = torch.device("cuda", 0)
    for priv, parent_of, paths, text in ((False, None, [[1, 2]] * 2999 + [[3, 2**32 - 5]], "hardened"),
                                         (False, [0] * 3000, [[1, 2]] * 1234 + [[H31, 2]] + [[1, 2]] * 1765, "hardened"),
                                         (True, [0] * 2999 + [1], [[1, H31]] * 3000, "parent index"),
                                         (False, [7] + [0] * 2999, [[1, 2]] * 3000, "parent index")):
        outs = [torch.full((w * 3000,), 0xAA, dtype=torch.uint8, device=dev) for w in WIDTHS]
        with pytest.raises(_native.BlsGpuError, match=text):
            _dev_call(engine, rec, priv, parent_of, paths, outs=outs)
        assert all(bool((o == 0xAA).all()) for o in outs), text
    outs = [torch.full((w * 8,), 0xAA, dtype=torch.uint8, device=dev) for w in WIDTHS]
    for depth, n_parents in ((0, 1), (256, 1), (2, 0)):
        with pytest.raises(_native.BlsGpuError):
            engine.hd_paths_dev(outs[2].data_ptr(), n_parents, True, None, outs[0].data_ptr(), depth, 1, outs[0].data_ptr(), outs[1].data_ptr(),
                                outs[2].data_ptr(), outs[3].data_ptr(), outs[4].data_ptr(), 0)
    engine.hd_paths_dev(outs[2].data_ptr(), 1, True, None, outs[0].data_ptr(), 2, 0, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                        outs[3].data_ptr(), outs[4].data_ptr(), 0)
    torch.cuda.synchronize()
    assert all(bool((o == 0xAA).all()) for o in outs)


def test_workspace_row_counts_in_the_total():
    from bls_py import _native
    e = _native.Engine(0)
    try:
        esk, _ = _keys()
        e.hd_paths(_record(esk), True, None, [[1]])           # builds the table
        before = e.workspace_bytes()
        e.hd_paths(_record(esk), False, None, [[1, 2]] * 5000)
        after = e.workspace_bytes()
        assert after["total"] >= before["total"] + 5000 * 256
        assert all(after[k] == before[k] for k in before if k not in ("total", "staging"))
    finally:
        e.close()
