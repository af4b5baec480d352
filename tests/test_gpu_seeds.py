"""Keys from seeds on the GPU: blsgpu_keys_from_seeds / blsgpu_keys_from_seeds_dev (csrc/blsgpu_seeds.hip k_seed_keys, one
seed per lane, then k_fix_mul_secret on the keys where it left them) against the reference's from_seed vectors
(tests/golden/seeds.json: every padding boundary of the HMAC, every class of the raw digest), against hmac and Python
integers, against blsgpu_g1_mul_gen of the same scalars, and chained on the device into blsgpu_hd_paths_secret_dev.

k_seed_keys and k_fix_mul_secret run 256 lanes per workgroup, 64 per wavefront: the counts sit on those boundaries +-1; the
_dev form cuts a call into slices of 2^20 seeds and the host form into staged slices of about 64 MB: one call crosses each."""
import ctypes
import random

import pytest

from bls_py import _native_seeds as S
from seeds_vectors import LENGTHS, N, by_length, expected, host_keys, load

pytestmark = pytest.mark.gpu

COUNTS = [1, 63, 64, 65, 257]
EINVAL = -22
WIDTHS = (32, 32, 96, 48, 160)          # key, chain code, affine, serialised, parent record


@pytest.fixture(scope="module")
def fx():
    return load()


@pytest.fixture(scope="module")
def drawn(engine):
    """for L = 32 and 56 and both modes: max(COUNTS) seeds from a fixed RNG -- seed i is the same whatever the size of the
    call -- with the keys and chain codes by hmac and Python integers and the public keys of those keys from
    blsgpu_g1_mul_gen, computed once"""
    out = {}
    for L in (32, 56):
        rnd = random.Random(0x5eed00 + L)
        seeds = [rnd.randbytes(L) for _ in range(max(COUNTS))]
        for hd in (False, True):
            keys = [host_keys(s, hd) for s in seeds]
            sks = b"".join(k[0] for k in keys)
            aff, ser = engine.g1_mul_gen(sks)
            out[L, hd] = {"seeds": b"".join(seeds), "sk": sks, "chain": b"".join(k[1] for k in keys) if hd else None, "aff": aff,
                          "ser": ser, "cls": {k[2] for k in keys}}
    return out


def parent_records(chain, aff, sk, n):
    return b"".join(chain[32 * i:32 * i + 32] + aff[96 * i:96 * i + 96] + sk[32 * i:32 * i + 32] for i in range(n))


@pytest.mark.parametrize("mode", ["plain", "hd"])
def test_every_fixture_length(engine, fx, mode):
    hd = mode == "hd"
    recs = by_length(fx)
    assert sorted(recs) == LENGTHS
    for L in LENGTHS:
        seeds = b"".join(bytes.fromhex(r["seed"]) for r in recs[L])
        got = S.keys_from_seeds(engine, seeds, L, len(recs[L]), hd, parents=hd)
        assert got == expected(recs[L], mode), L


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("hd", [False, True])
@pytest.mark.parametrize("L", [32, 56])
def test_counts_against_the_host(engine, drawn, L, hd, n):
    d = drawn[L, hd]
    assert d["cls"] == {0, 1, 2}                                 # every class of the raw digest among the lanes
    sk, chain, aff, ser, par = S.keys_from_seeds(engine, d["seeds"][:L * n], L, n, hd, parents=hd)
    assert sk == d["sk"][:32 * n] and all(int.from_bytes(sk[32 * i:32 * i + 32], "big") < N for i in range(n))
    assert aff == d["aff"][:96 * n] and ser == d["ser"][:48 * n]
    if hd:
        assert chain == d["chain"][:32 * n] and par == parent_records(chain, aff, sk, n)
    else:
        assert chain is None and par is None


@pytest.mark.parametrize("hd", [False, True])
def test_each_output_alone(engine, drawn, hd):
    L, n = 56, 65
    d = drawn[L, hd]
    seeds = d["seeds"][:L * n]
    full = S.keys_from_seeds(engine, seeds, L, n, hd, parents=hd)
    flags = ("sk", "chain", "aff", "ser", "parents")
    for k, name in enumerate(flags):
        if full[k] is None:
            continue
        only = S.keys_from_seeds(engine, seeds, L, n, hd, **{f: f == name for f in flags})
        assert only == tuple(v if j == k else None for j, v in enumerate(full)), name


def test_dev_form_feeds_the_path_kernel(engine, fx):
    """seeds -> out_parents -> blsgpu_hd_paths_secret_dev on one stream, the records never leaving the device: the leaves are
    the fixture's path leaves (private_child of the reference folded over the path)"""
    import torch
    dev = torch.device("cuda", 0)
    want = fx["paths"]
    seeds = [bytes.fromhex(p["seed"]) for p in want]
    assert [len(s) for s in seeds] == [32] * 4 + [64] * 4
    n, depth = len(seeds), len(fx["path"])
    d_seeds = torch.frombuffer(bytearray(b"".join(seeds)), dtype=torch.uint8).to(dev)
    d_of = torch.arange(n, dtype=torch.int32, device=dev)
    d_idx = torch.tensor(fx["path"] * n, dtype=torch.int64, device=dev).to(torch.int32)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        d_par = torch.full((160 * (n + 1),), 0xAA, dtype=torch.uint8, device=dev)
        outs = [torch.full((w * n,), 0xAA, dtype=torch.uint8, device=dev) for w in (32, 32, 96, 48, 4)]
        S.keys_from_seeds_dev(engine, d_seeds.data_ptr(), 32, 4, True, None, None, None, None, d_par.data_ptr(), stream.cuda_stream)
        S.keys_from_seeds_dev(engine, d_seeds.data_ptr() + 32 * 4, 64, 4, True, None, None, None, None, d_par.data_ptr() + 160 * 4,
                              stream.cuda_stream)
        engine.hd_paths_secret_dev(d_par.data_ptr(), n, d_of.data_ptr(), d_idx.data_ptr(), depth, n, *[o.data_ptr() for o in outs],
                                   stream.cuda_stream)
    stream.synchronize()
    chain, sk, aff, ser, fp = (bytes(o.cpu().numpy()) for o in outs)
    leaves = [(1).to_bytes(4, "big") + bytes([depth]) + fp[4 * i:4 * i + 4] + fx["path"][-1].to_bytes(4, "big") + chain[32 * i:32 * i + 32]
              + sk[32 * i:32 * i + 32] for i in range(n)]
    assert [v.hex() for v in leaves] == [p["leaf"] for p in want]
    assert [ser[48 * i:48 * i + 48].hex() for i in range(n)] == [p["leaf_pk"] for p in want]
    # the records are the masters of the fixture, and the one behind the last is untouched
    recs = {r["seed"]: r["hd"] for r in fx["seeds"]}
    par = bytes(d_par.cpu().numpy())
    assert par[:160 * n].hex() == "".join(recs[p["seed"]]["chain"] + recs[p["seed"]]["aff"] + recs[p["seed"]]["sk"] for p in want)
    assert par[160 * n:] == b"\xaa" * 160


def test_dev_form_every_output_on_a_stream(engine, drawn):
    import torch
    dev = torch.device("cuda", 0)
    L, n = 32, 257
    d = drawn[L, True]
    d_seeds = torch.frombuffer(bytearray(d["seeds"][:L * n]), dtype=torch.uint8).to(dev)
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        outs = [torch.full((w * (n + 1),), 0xAA, dtype=torch.uint8, device=dev) for w in WIDTHS]
        S.keys_from_seeds_dev(engine, d_seeds.data_ptr(), L, n, True, *[o.data_ptr() for o in outs], stream.cuda_stream)
    stream.synchronize()
    got = [bytes(o.cpu().numpy()) for o in outs]
    want = [d["sk"][:32 * n], d["chain"][:32 * n], d["aff"][:96 * n], d["ser"][:48 * n]]
    want.append(parent_records(want[1], want[2], want[0], n))
    # the spare lanes of the last workgroup store nothing: the item behind the last one is untouched
    assert got == [v + b"\xaa" * w for v, w in zip(want, WIDTHS)]


def _sampled(n, cuts):
    return sorted({i for c in [0, n] + list(cuts) for i in range(c - 2, c + 2) if 0 <= i < n})


def test_dev_form_across_its_slices(engine):
    """2^20 + 3 seeds in the hd form with the records as the only output: keys and affine keys of every slice pass through the
    workspace.  Sampled at both ends and on either side of the cut."""
    import torch
    dev = torch.device("cuda", 0)
    L, n = 8, (1 << 20) + 3
    g = torch.Generator().manual_seed(0x5eed)
    seeds = torch.randint(0, 256, (L * n,), dtype=torch.uint8, generator=g)
    host = bytes(seeds.numpy())
    d_seeds = seeds.to(dev)
    d_par = torch.full((160 * n + 160,), 0xAA, dtype=torch.uint8, device=dev)
    S.keys_from_seeds_dev(engine, d_seeds.data_ptr(), L, n, True, None, None, None, None, d_par.data_ptr(), 0)
    torch.cuda.synchronize(dev)
    par = bytes(d_par.cpu().numpy())
    assert par[160 * n:] == b"\xaa" * 160
    pos = _sampled(n, [1 << 20])
    keys = [host_keys(host[L * i:L * i + L], True) for i in pos]
    aff, _ = engine.g1_mul_gen(b"".join(k[0] for k in keys))
    for t, i in enumerate(pos):
        assert par[160 * i:160 * i + 160] == keys[t][1] + aff[96 * t:96 * t + 96] + keys[t][0], i


def test_host_form_across_its_staged_slices(engine):
    """seeds of the longest length, more than one staged slice of them (2^26 / (1024 + 368) = 48 210 per slice), keys only"""
    L = 1024
    per = (1 << 26) // (L + 368)
    n = per + 70
    seeds = random.Random(0x5eed1).randbytes(L * n)
    sk = S.keys_from_seeds(engine, seeds, L, n, False, aff=False, ser=False)[0]
    assert len(sk) == 32 * n
    for i in _sampled(n, [per]):
        assert sk[32 * i:32 * i + 32] == host_keys(seeds[L * i:L * i + L], False)[0], i


def test_argument_errors_leave_the_outputs_untouched(engine):
    L = engine.lib
    seeds = bytes(range(40))
    outs = [ctypes.create_string_buffer(b"\xAA" * (w * 5), w * 5) for w in WIDTHS]
    o = [ctypes.cast(b, ctypes.c_void_p) for b in outs]
    F, D = L.blsgpu_keys_from_seeds, L.blsgpu_keys_from_seeds_dev

    def refused(rc):
        assert rc == EINVAL and L.blsgpu_last_error()
    refused(F(engine.h, bytes(1025 * 5), 1025, 5, 1, *o))                    # seed_len above the limit
    refused(F(engine.h, bytes(1025 * 5), 1025, 5, 0, o[0], None, o[2], o[3], None))
    refused(F(engine.h, None, 8, 5, 1, *o))                                  # no seeds
    refused(F(engine.h, seeds, 8, 5, 1, None, None, None, None, None))       # no output
    refused(F(engine.h, seeds, 8, 5, 0, None, None, None, None, None))
    for hd in (2, -1):
        refused(F(engine.h, seeds, 8, 5, hd, *o))
    refused(F(engine.h, seeds, 8, 5, 0, o[0], o[1], o[2], o[3], None))       # a chain code outside the hd form
    refused(F(engine.h, seeds, 8, 5, 0, o[0], None, o[2], o[3], o[4]))       # parent records outside the hd form
    refused(F(None, seeds, 8, 5, 1, *o))
    assert all(b.raw == b"\xAA" * len(b.raw) for b in outs)
    # the same checks guard the device form (no launch is made: the pointers are never used)
    refused(D(engine.h, None, 8, 5, 1, *o, None))
    refused(D(engine.h, o[0], 1025, 5, 1, *o, None))
    refused(D(engine.h, o[0], 8, 5, 2, *o, None))
    refused(D(engine.h, o[0], 8, 5, 0, o[0], o[1], None, None, None, None))
    refused(D(engine.h, o[0], 8, 5, 1, None, None, None, None, None, None))
    with pytest.raises(ValueError):
        S.keys_from_seeds(engine, bytes(1025), 1025, 1)
    with pytest.raises(ValueError):
        S.keys_from_seeds(engine, seeds, 8, 4)
    with pytest.raises(ValueError):
        S.keys_from_seeds(engine, seeds, 8, 5, False, parents=True)


def test_empty_calls_and_empty_seeds(engine):
    L = engine.lib
    buf = ctypes.create_string_buffer(b"\xAA" * 8, 8)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.blsgpu_keys_from_seeds(engine.h, None, 32, 0, 1, p, p, p, p, p) == 0
    assert L.blsgpu_keys_from_seeds(engine.h, None, 0, 0, 0, None, None, None, None, None) == 0
    assert L.blsgpu_keys_from_seeds_dev(engine.h, None, 32, 0, 1, None, None, None, None, None, None) == 0
    assert buf.raw == b"\xAA" * 8
    assert S.keys_from_seeds(engine, b"", 32, 0, True, parents=True) == (b"", b"", b"", b"", b"")
    # seed_len == 0: the reference accepts b""; seeds may be NULL (the marshalling hands NULL over)
    for hd in (False, True):
        sk, chain, aff, ser, _ = S.keys_from_seeds(engine, b"", 0, 3, hd)
        want = host_keys(b"", hd)
        assert sk == want[0] * 3 and (chain == want[1] * 3 if hd else chain is None)
        assert (aff, ser) == engine.g1_mul_gen(want[0] * 3)


def test_timing_kinds(engine, drawn):
    d = drawn[32, True]
    engine.timing_enable(True)
    try:
        engine.timing_read()
        S.keys_from_seeds(engine, d["seeds"][:32 * 65], 32, 65, True, parents=True)
        kinds = [k for k, _ in engine.timing_read()]
        assert kinds == [13, 9]                                              # k_seed_keys, then the multiplication
        S.keys_from_seeds(engine, d["seeds"][:32 * 65], 32, 65, True, aff=False, ser=False)
        assert [k for k, _ in engine.timing_read()] == [13]                  # no public key asked for: no multiplication
    finally:
        engine.timing_enable(False)


def test_workspace_is_counted_in_the_total(drawn):
    """a fresh context, the records as the only output: the keys and the affine keys lie in the workspace, which the total
    counts (a grow-only buffer takes a quarter of headroom) beside the signed-window table"""
    from bls_py import _native
    e = _native.Engine(0)
    try:
        n = 300
        before = e.workspace_bytes()
        par = S.keys_from_seeds(e, drawn[32, True]["seeds"][:32 * 257] + bytes(32 * 43), 32, n, True, sk=False, chain=False, aff=False,
                                ser=False, parents=True)[4]
        after = e.workspace_bytes()
        held = n * (32 + 96)
        assert after["total"] - before["total"] - (after["staging"] - before["staging"]) == 58240 + held + held // 4
        d = drawn[32, True]
        assert par[:160 * 257] == parent_records(d["chain"], d["aff"], d["sk"], 257)
    finally:
        e.close()
