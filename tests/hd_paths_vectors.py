"""Shared by tests/test_hd_paths_host.py and tests/test_gpu_hd_paths.py: the HD path vectors of
tests/golden/hd_paths.json (generated from the reference by tests/golden/make_golden_hd_paths.py) checked through
whatever provider bls_py.backend holds, and a host-only provider of hd_paths (tests/hd_vectors.HostHD chained level by
level) for the CPU tests."""
import hashlib

from bls_py import hostmath as H
from hd_vectors import HostHD


class HostHDPaths(HostHD):
    """HostHD with hd_paths of bls_py.backend.HipProvider on the host: `depth` chained hd_children steps per path, the
    fingerprint of the last parent by hashlib -- the defining property of blsgpu_hd_paths, no GPU."""

    def hd_paths(self, parents, priv, parent_of, paths):
        self.calls.append(("hd_paths", len(paths), len(paths[0]) if paths else 0))
        calls = self.calls
        self.calls = []                                    # (the chained steps below are not calls of the surface under test)
        out = [[], [], [], [], []]
        try:
            for j, path in enumerate(paths):
                rec = parents[160 * (parent_of[j] if parent_of is not None else 0):][:160]
                chain, aff, sk = rec[:32], rec[32:128], rec[128:] if priv else None
                for i in path:
                    fp = hashlib.sha256(H.g1_compress(H.g1_from_abi(aff))).digest()[:4]
                    c, s, a, ser = self.hd_children(chain, aff, sk, [i])
                    chain, aff, sk = c, a, s
                for o, v in zip(out, (chain, sk, aff, ser, fp)):
                    o.append(v)
        finally:
            self.calls = calls
        return (b"".join(out[0]), b"".join(out[1]) if priv else None, b"".join(out[2]), b"".join(out[3]), b"".join(out[4]))


def check_digest(sers, rec, full=True):
    """serialisations against a fixture record {count, sha256, every16}; not full: the sampled positions only (`sers` then
    holds exactly those, in order)"""
    pos = sorted(int(k) for k in rec["every16"])
    if full:
        assert len(sers) == rec["count"]
        assert hashlib.sha256(b"".join(sers)).hexdigest() == rec["sha256"]
        sers = [sers[k] for k in pos]
    assert [s.hex() for s in sers] == [rec["every16"][str(k)] for k in pos]


def _pick(rec, paths, full):
    return paths if full else [paths[int(k)] for k in sorted(int(k) for k in rec["every16"])]


def check_private_record(rec, full=True):
    from bls_py.keys import ExtendedPrivateKey
    esk = ExtendedPrivateKey.from_seed(bytes.fromhex(rec["seed"]))
    paths = _pick(rec["esk"], rec["paths"], full)
    leaves = esk.private_path_batch(paths)
    check_digest([k.serialize() for k in leaves], rec["esk"], full)
    check_digest([k.get_extended_public_key().serialize() for k in leaves], rec["epk"], full)
    check_digest([k.serialize() for k in esk.public_path_batch(paths)], rec["epk"], full)
    for k, p in zip(leaves, paths):
        assert k.depth == len(p) and k.child_number == p[-1]
        assert k.get_public_key() == k.get_extended_public_key().public_key      # the caches hold the key of the leaf


def check_public_record(rec, full=True):
    from bls_py.keys import ExtendedPublicKey
    xpub = ExtendedPublicKey.from_bytes(bytes.fromhex(rec["xpub"]))
    paths = _pick(rec["epk"], rec["paths"], full)
    leaves = xpub.public_path_batch(paths)
    check_digest([k.serialize() for k in leaves], rec["epk"], full)
    for k, p in zip(leaves, paths):
        assert k.depth == xpub.depth + len(p) and k.child_number == p[-1]


def check_grid_record(rec, full=True):
    """the m/a/i grid: accounts as paths of length 1, then every address of every account from its own parent in one call"""
    from bls_py.keys import ExtendedPublicKey
    root = ExtendedPublicKey.from_bytes(bytes.fromhex(rec["xpub"]))
    A, I = rec["accounts"], rec["addresses"]
    accounts = root.public_path_batch([[a] for a in range(A)])
    check_digest([k.serialize() for k in accounts], rec["parents"], True)
    cells = [(a, i) for a in range(A) for i in range(I)]
    if not full:
        cells = [cells[int(k)] for k in sorted(int(k) for k in rec["epk"]["every16"])]
    leaves = ExtendedPublicKey.public_paths_from(accounts, [a for a, _ in cells], [[i] for _, i in cells])
    check_digest([k.serialize() for k in leaves], rec["epk"], full)
    # the same leaves as paths of length 2 from the root
    two = root.public_path_batch([[a, i] for a, i in cells])
    assert [k.serialize() for k in two] == [k.serialize() for k in leaves]
