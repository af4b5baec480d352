"""Subgroup membership kernels (csrc/blsgpu_subgroup.hip) and BLS.verify_batch_randomized on the GPU.  The expected verdicts
are the reference's own (P * n).infinity, read from tests/golden/subgroup.json.  Needs an MI355X."""
import ctypes
import random

import pytest

from subgroup_vectors import aggregates, expected_status, secret_keys

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def hip_provider(engine):
    from bls_py import backend
    backend.use(None)          # default HIP provider
    assert type(backend.get()).__name__ == "HipProvider"
    yield


@pytest.fixture(scope="module")
def sub(golden):
    return golden("subgroup.json")


GROUPS = (("g1", 96), ("g2", 192))


def _points(sub, g):
    return [bytes.fromhex(r["point"]) for r in sub[g]], bytes(expected_status(r) for r in sub[g])


@pytest.mark.parametrize("g,psz", GROUPS)
def test_each_point_alone(engine, sub, g, psz):
    pts, want = _points(sub, g)
    fn = getattr(engine, g + "_subgroup")
    assert bytes(fn(p)[0] for p in pts) == want
    assert set(want) == {0, 1, 2}


@pytest.mark.parametrize("g,psz", GROUPS)
@pytest.mark.parametrize("n", [100, 65536])
def test_shuffled_repeats(engine, sub, g, psz, n):
    """n = 100: one full wavefront and a partly filled one; n = 65536: the fixture points repeated in a shuffled order"""
    pts, want = _points(sub, g)
    idx = [i % len(pts) for i in range(n)]
    random.Random(n).shuffle(idx)
    got = getattr(engine, g + "_subgroup")(b"".join(pts[i] for i in idx))
    assert got == bytes(want[i] for i in idx)


@pytest.mark.parametrize("g,psz", GROUPS)
def test_dev_form_matches_host_form(engine, sub, g, psz):
    import torch
    pts, want = _points(sub, g)
    buf = b"".join(pts) * 3
    n = len(buf) // psz
    d_pts = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    d_st = torch.full((n + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    getattr(engine, g + "_subgroup_dev")(d_pts.data_ptr(), n, d_st.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    st = bytes(d_st.cpu().tolist())
    assert st[:n] == want * 3
    assert st[n:] == b"\xab" * 64                                  # nothing written past n


@pytest.mark.parametrize("g,psz", GROUPS)
def test_einval_before_anything_is_written(engine, g, psz):
    lib, h = engine.lib, engine.h
    host, dev = getattr(lib, "blsgpu_%s_subgroup_check" % g), getattr(lib, "blsgpu_%s_subgroup_check_dev" % g)
    st = ctypes.create_string_buffer(b"\x07" * 4, 4)
    assert host(h, None, 1, st) == -22
    assert host(h, bytes(psz), 1, None) == -22
    assert st.raw == b"\x07" * 4
    assert dev(h, None, 1, None, None) == -22
    assert host(h, None, 0, None) == 0 and dev(h, None, 0, None, None) == 0
    assert host(h, bytes(psz), 1, st) == 0 and st.raw[0] == 1        # the all-zero encoding: infinity, in the subgroup


def test_in_subgroup_batch(sub):
    from bls_py import hostmath as H
    from bls_py.ec import JacobianPoint, default_ec, default_ec_twist
    from bls_py.keys import PublicKey
    from bls_py.signature import Signature
    keys = [PublicKey(JacobianPoint._from(H.F1, H.aff_to_jac(H.F1, H.g1_from_abi(bytes.fromhex(r["point"]))), default_ec))
            for r in sub["g1"]]
    sigs = [Signature(JacobianPoint._from(H.F2, H.aff_to_jac(H.F2, H.g2_from_abi(bytes.fromhex(r["point"]))), default_ec_twist))
            for r in sub["g2"]]
    assert PublicKey.in_subgroup_batch(keys) == [r["in_subgroup"] for r in sub["g1"]]
    assert Signature.in_subgroup_batch(sigs) == [r["in_subgroup"] for r in sub["g2"]]


@pytest.mark.parametrize("forged_at", [None, 2])
def test_randomized_matches_verify_batch_C2(forged_at):
    """the C2 shape of tests/test_gpu_scheme.py (sign -> aggregate -> verify), 6 aggregates of 40, with and without a forgery,
    plus single signatures"""
    from bls_py.bls import BLS
    from bls_py.keys import PrivateKey
    batch = aggregates(6, 40, forged_at) + PrivateKey.sign_batch(secret_keys(b"single", 2), [b"one", b"two"])
    want = BLS.verify_batch(batch)
    assert want == [i != forged_at for i in range(8)]
    assert BLS.verify_batch_randomized(batch, rng=random.Random(3)) == want
    assert BLS.verify_batch_randomized(batch) == want                 # the default rng


def test_randomized_4096_signatures_over_16_messages():
    from bls_py.bls import BLS
    from bls_py.keys import PrivateKey
    sks = secret_keys(b"committee", 4096)
    sigs = PrivateKey.sign_batch(sks, [b"slot %d" % (i % 16) for i in range(4096)])
    want = BLS.verify_batch(sigs)
    assert want == [True] * 4096
    assert BLS.verify_batch_randomized(sigs, rng=random.Random(5)) == want
    sigs[1000] = sks[1000].sign(b"slot 99")
    sigs[1000].set_aggregation_info(sigs[1016].aggregation_info)
    want = BLS.verify_batch(sigs)
    assert want == [i != 1000 for i in range(4096)]
    assert BLS.verify_batch_randomized(sigs, rng=random.Random(6)) == want
