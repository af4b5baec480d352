"""The pairing_multi_ranges extension without a GPU: a recording host provider (tests/subgroup_vectors.HostRLC) that offers it, its
ranges computed by the CPU oracle; BLS.verify_batch(ragged=True) against verify_batch() on a mixed batch, with exactly one
extension call; the default path's calls unchanged, extension or not; a provider without the extension raises; and the argument
validation of bls_py._native_pairranges."""
import pytest

from subgroup_vectors import HostRLC
from test_msmr_host import world                                             # noqa: F401  (the ragged, forged and uniform aggregates)


class WithExtension(HostRLC):
    """a stand-in that offers the extension as a stand-in does: an attribute of that name"""

    def pairing_multi_ranges(self, g1, g2, ranges, inf=None):
        self.calls.append(("pairing_multi_ranges", len(g1) // 96, list(ranges)))
        return b"".join(self.O.pairing_multi(g1[96 * b:96 * e], g2[192 * b:192 * e], e - b, threads=8,
                                             inf=None if inf is None else inf[2 * b:2 * e]) for b, e in ranges)


@pytest.fixture
def use(oracle):
    from bls_py import backend
    old = backend._provider

    def install(cls):
        p = cls(oracle)
        backend.use(p)
        return p
    yield install
    backend.use(old)


def pairings(p):
    return [c for c in p.calls if c[0].startswith("pairing_multi")]


def test_ragged_equals_the_default_with_one_extension_call(use, world):                      # noqa: F811
    """ragged (5 pairs: one message of 4 signers, three of 1, and the signature), a forged copy, uniform (3 pairs): one pair list
    of 13 pairs, -G1 / sig first in every range"""
    from bls_py import backend
    from bls_py.bls import BLS
    ragged, forged, uniform = world
    batch = [ragged, forged, uniform, ragged]
    p = use(WithExtension)
    assert backend.extension("pairing_multi_ranges") is not None
    want = BLS.verify_batch(batch)
    assert want == [True, False, True, True]
    default_calls = pairings(p)
    assert sorted(default_calls) == [("pairing_multi_batch", 3, 1), ("pairing_multi_batch", 5, 3)]
    p.calls.clear()
    assert BLS.verify_batch(batch, ragged=True) == want
    assert pairings(p) == [("pairing_multi_ranges", 18, [(0, 5), (5, 10), (10, 13), (13, 18)])]
    # everything before the pairing is the default path's
    others = [c[0] for c in p.calls if not c[0].startswith("pairing_multi")]
    p.calls.clear()
    BLS.verify_batch(batch)
    assert [c[0] for c in p.calls if not c[0].startswith("pairing_multi")] == others
    assert BLS.verify_batch([], ragged=True) == []


def test_the_default_path_takes_exactly_the_calls_it_took(use, world):                       # noqa: F811
    """with the extension present, verify_batch() -- and verify and verify_batch_randomized -- make the calls of a provider
    without it: nothing is routed through the ranges call"""
    import random
    from bls_py.bls import BLS
    batch = list(world)
    seen = []
    for cls in (HostRLC, WithExtension):
        p = use(cls)
        got = [BLS.verify(s) for s in batch], BLS.verify_batch(batch), BLS.verify_batch(batch, ragged=False), \
            BLS.verify_batch_randomized(batch, rng=random.Random(3))
        assert got == ([True, False, True],) * 4
        seen.append([c[:3] for c in p.calls])
    assert seen[0] == seen[1] and all(c[0] != "pairing_multi_ranges" for c in seen[1])
    assert ("pairing_multi_batch", 5, 2) in seen[0] and ("pairing_multi_batch", 3, 1) in seen[0]


def test_a_provider_without_the_extension_raises(use, world):                                # noqa: F811
    from bls_py import backend
    from bls_py.bls import BLS
    p = use(HostRLC)
    assert backend.extension("pairing_multi_ranges") is None
    with pytest.raises(NotImplementedError):
        BLS.verify_batch(list(world), ragged=True)
    assert p.calls == []                                                     # raised before any work
    assert backend.PAIR_RANGE_EXTENSIONS == {"pairing_multi_ranges": "_native_pairranges"}


class FakeEngine:
    """_native.Engine's marshalling helpers over a device call that must not happen"""

    def __init__(self):
        from bls_py import _native
        self._indices = _native.Engine._indices
        self.calls = []

    def _call_out(self, name, *args, out, tail=()):
        self.calls.append((name, args[2], args[3], list(args[4]), args[5], out))
        return [bytes(size) for size in out]

    def _call(self, name, *args):
        self.calls.append((name,) + args[:4] + (list(args[4]),) + args[5:])


def test_argument_validation_raises_before_any_device_call():
    from bls_py import _native, _native_pairranges as R
    eng = FakeEngine()
    g1, g2 = bytes(96 * 3), bytes(192 * 3)
    with pytest.raises(ValueError):
        R.pairing_multi_ranges(eng, g1[:-1], g2, [(0, 3)])                   # not whole points
    with pytest.raises(ValueError):
        R.pairing_multi_ranges(eng, g1, g2[:-192], [(0, 3)])                 # a G2 point per G1 point
    with pytest.raises(ValueError):
        R.pairing_multi_ranges(eng, g1, g2, [(0, 3)], inf=bytes(5))          # two flags per pair
    with pytest.raises(ValueError):
        R.pairing_multi_ranges(eng, g1, g2, [(0, 3), (1,)])                  # a range is a pair
    with pytest.raises(ValueError):
        R.pairing_multi_ranges(eng, g1, g2, [(-1, 3)])
    with pytest.raises(OverflowError):
        R.pairing_multi_ranges(eng, g1, g2, [(0, 1 << 32)])                  # 32-bit indices
    assert eng.calls == []
    assert R.pairing_multi_ranges(eng, g1, g2, [(0, 3), (1, 1)], inf=bytes(6)) == bytes(2 * 576)
    assert R.pairing_multi_ranges(eng, g1, g2, []) == b""
    assert eng.calls == [("blsgpu_pairing_multi_ranges", bytes(6), 3, [0, 3, 1, 1], 2, [1152]),
                         ("blsgpu_pairing_multi_ranges", None, 3, [0], 0, [0])]
    eng.calls.clear()
    R.pairing_multi_ranges_dev(eng, 1, 2, 3, [(0, 3), (2, 2)], 5)
    R.pairing_multi_ranges_dev(eng, 1, 2, 3, [(0, 1)], 5, stream=9, d_inf=7)
    assert eng.calls == [("blsgpu_pairing_multi_ranges_dev", 1, 2, None, 3, [0, 3, 2, 2], 2, 5, 0),
                         ("blsgpu_pairing_multi_ranges_dev", 1, 2, 7, 3, [0, 1], 1, 5, 9)]
    assert {"blsgpu_pairing_multi_ranges", "blsgpu_pairing_multi_ranges_dev"} <= set(_native.PROTOTYPES)
