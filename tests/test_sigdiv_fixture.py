"""Signature.divide_by and Signature.divide_by_batch without a GPU: the mirror's divide_by against the reference's results
(tests/golden/sigdiv.json), the batch under a provider without the `sig_divide` extension (the loop) and under a host stand-in
for it (tests/sigdiv_vectors.HostSigDivide), where the routing, the trees and the order of the errors are the batch's own."""
import pytest

from bls_py import backend
from bls_py.signature import Signature
from sigdiv_vectors import NOT_UNIQUE, HostSigDivide, N, case_objects, expected_of, outcome, record_of

NAMES = ["nested_three_leaves", "empty_divisor_list", "not_a_subset", "nested_one_leaf", "not_unique", "by_aggregate",
         "secure_one_leaf", "secure_two_leaves", "all_parts"]


@pytest.fixture(scope="module")
def cases(golden):
    cs = golden("sigdiv.json")
    assert [c["name"] for c in cs] == NAMES
    return [(c, case_objects(c)) for c in cs]


@pytest.fixture()
def provider():
    """installs a provider for one test and puts the previous one back"""
    old = backend._provider

    def install(p):
        backend.use(p)
        return p
    yield install
    backend.use(old)


def test_fixture_covers_what_it_should(cases):
    by = {c["name"]: c for c, _ in cases}
    assert by["not_a_subset"]["error"] == "Signature is not a subset" and by["not_unique"]["error"] == NOT_UNIQUE
    assert by["all_parts"]["result"]["tree"] == [] and by["empty_divisor_list"]["divisors"] == []
    quotients = lambda c: {int(a[2], 16) * pow(int(b[2], 16), -1, N) % N
                           for d in c["divisors"] for b in d["tree"] for a in c["dividend"]["tree"] if a[:2] == b[:2]}
    assert 1 not in quotients(by["secure_one_leaf"]) and len(quotients(by["secure_two_leaves"])) == 2
    assert quotients(by["all_parts"]) == {1}                 # the plain path's case; every other aggregate was merged securely
    assert all(c["verify"] for c, _ in cases if c.get("verify") is not None)


def test_mirror_divide_by_reproduces_the_reference(cases):
    for c, (dividend, divisors) in cases:
        assert outcome(lambda: [dividend.divide_by(divisors)]) == expected_of(c), c["name"]


def test_batch_without_the_extension_is_the_loop(cases, provider):
    provider(object())                                       # offers nothing: extension("sig_divide") is None
    good = [(c, o) for c, o in cases if "error" not in c]
    got = Signature.divide_by_batch([d for _, (d, _) in good], [ds for _, (_, ds) in good])
    assert [record_of(s) for s in got] == [c["result"] for c, _ in good]
    for c, (dividend, divisors) in cases:
        assert outcome(lambda: Signature.divide_by_batch([dividend], [divisors])) == expected_of(c), c["name"]
    assert Signature.divide_by_batch([], []) == []
    with pytest.raises(ValueError):
        Signature.divide_by_batch([cases[0][1][0]], [])


def test_batch_on_a_host_stand_in_for_the_extension(cases, provider):
    p = provider(HostSigDivide())
    good = [(c, o) for c, o in cases if "error" not in c]
    dividends, lists = [d for _, (d, _) in good], [ds for _, (_, ds) in good]
    got = Signature.divide_by_batch(dividends, lists)
    assert [record_of(s) for s in got] == [c["result"] for c, _ in good]
    # one call: every dividend's own point plus its divisors, every divisor's entries
    assert p.calls == [(len(good), sum(1 + len(ds) for ds in lists), sum(len(d["tree"]) for c, _ in good for d in c["divisors"]))]
    for s, d in zip(got, dividends):                         # a fresh info: nothing of the dividend's is shared or cached
        assert s.aggregation_info is not d.aggregation_info and s.aggregation_info.tree is not d.aggregation_info.tree
        assert "_okey" not in s.aggregation_info.__dict__
    for c, (dividend, divisors) in cases:
        assert outcome(lambda: Signature.divide_by_batch([dividend], [divisors])) == expected_of(c), c["name"]


def test_batch_raises_the_first_failing_dividend_in_input_order(cases, provider):
    by = {c["name"]: o for c, o in cases}
    ok, subset, unique = by["nested_one_leaf"], by["not_a_subset"], by["not_unique"]
    loop = lambda ds: outcome(lambda: [d.divide_by(v) for d, v in ds])
    for order in ([ok, unique, subset], [ok, subset, unique], [subset, ok], [unique, ok], [ok, ok]):
        p = provider(HostSigDivide())
        got = outcome(lambda: Signature.divide_by_batch([d for d, _ in order], [v for _, v in order]))
        assert got == loop(order)
        # a failing lookup in the first dividend is raised before any device call
        assert (p.calls == []) == (order[0] is subset)
    # inside ONE dividend the loop meets a non-unique divisor before a later divisor that is no subset, and the other way round
    final, sig_l = unique[0], unique[1][0]
    stranger = by["not_a_subset"][1][0]
    quotient = by["not_a_subset"][0]
    for dividend, divisors in ((final, [sig_l, stranger]), (quotient, [stranger, sig_l])):
        provider(HostSigDivide())
        assert outcome(lambda: Signature.divide_by_batch([dividend], [divisors])) == loop([(dividend, divisors)])


def test_divisors_with_an_empty_info_are_skipped_and_zero_exponents_go_to_the_loop(cases, provider):
    from bls_py.aggregation_info import AggregationInfo
    by = {c["name"]: o for c, o in cases}
    dividend, divisors = by["nested_three_leaves"]
    empty = Signature(divisors[0].value, AggregationInfo._from_tree({}))
    p = provider(HostSigDivide())
    got = Signature.divide_by_batch([dividend], [[empty] + divisors + [empty]])
    assert record_of(got[0]) == record_of(dividend.divide_by([empty] + divisors + [empty])) == record_of(dividend.divide_by(divisors))
    assert p.calls == [(1, 1 + len(divisors), 3)]
    # a divisor exponent that is 0 mod n: the device does not decide it (status 2), the host loop's result stands
    key = next(iter(divisors[1].aggregation_info.tree))
    zero = Signature(divisors[1].value, AggregationInfo._from_tree({key: N}))
    want = outcome(lambda: [dividend.divide_by([divisors[0], zero])])
    assert outcome(lambda: Signature.divide_by_batch([dividend], [[divisors[0], zero]])) == want
