"""util.hash256_batch without a GPU: under a provider that has no hash256 extension (the host provider of the CPU tests) the
batch form is exactly the loop; under a stand-in that offers one, the extension gets the messages and its bytes are cut into
digests."""
import hashlib

import pytest

from bls_py import backend, util

MESSAGES = [b"", b"a", b"abc" * 40, bytes(range(256)) * 5, b"\x00" * 55, b"\x00" * 56, b"\x00" * 64]


@pytest.fixture
def provider():
    old = backend._provider

    def use(p):
        backend.use(p)
        return p
    yield use
    backend.use(old)


def test_host_provider_is_the_loop(provider):
    provider(object())                                                       # no extension of any name
    assert backend.extension("hash256") is None
    assert util.hash256_batch(MESSAGES) == [util.hash256(m) for m in MESSAGES] == [hashlib.sha256(m).digest() for m in MESSAGES]
    assert util.hash256_batch([]) == [] and util.hash256_batch(iter(())) == []
    assert util.hash256_batch(["abc", b"abc"]) == [util.hash256("abc")] * 2


def test_bytes_bytearray_memoryview(provider):
    provider(object())
    want = [hashlib.sha256(m).digest() for m in MESSAGES]
    assert util.hash256_batch([bytearray(m) for m in MESSAGES]) == want
    assert util.hash256_batch([memoryview(m) for m in MESSAGES]) == want
    assert util.hash256_batch([memoryview(b"xx" + m + b"y")[2:-1] for m in MESSAGES]) == want
    assert util.hash256_batch(m for m in MESSAGES) == want


def test_extension_is_taken_when_offered(provider):
    class StandIn:
        def __init__(self):
            self.seen = []

        def hash256(self, messages):
            self.seen.append(list(messages))
            return b"".join(hashlib.sha256(m).digest() for m in messages)
    p = provider(StandIn())
    assert util.hash256_batch(MESSAGES) == [hashlib.sha256(m).digest() for m in MESSAGES] and p.seen == [MESSAGES]
    assert util.hash256_batch([]) == [] and len(p.seen) == 1                 # an empty list never reaches the provider
