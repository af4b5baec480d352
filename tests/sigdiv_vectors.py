"""Shared by the Signature.divide_by tests: the objects of tests/golden/sigdiv.json (make_golden_sigdiv.py) rebuilt on the
mirror's classes, the expected scalars and statuses of blsgpu_sig_divide from Python integers, and a host stand-in for the
`sig_divide` extension so the batch method's routing runs without a GPU."""
from bls_py import hostmath as H
from bls_py.aggregation_info import AggregationInfo
from bls_py.keys import PublicKey
from bls_py.signature import Signature

N = H.N
NOT_UNIQUE = "Cannot divide by aggregate signature,msg/pk pairs are not unique"


def signature_of(rec, keys=None):
    """the mirror's Signature of a fixture record {sig, tree}; keys: a cache hex -> PublicKey shared by a case"""
    keys = {} if keys is None else keys
    tree = {}
    for mh, pk, e in rec["tree"]:
        if pk not in keys:
            keys[pk] = PublicKey.from_bytes(bytes.fromhex(pk))
        tree[(bytes.fromhex(mh), keys[pk])] = int(e, 16)
    return Signature.from_bytes(bytes.fromhex(rec["sig"]), AggregationInfo._from_tree(tree))


def record_of(sig):
    """a Signature in the fixture's form"""
    info = sig.aggregation_info
    return {"sig": sig.serialize().hex(),
            "tree": [[mh.hex(), pk.serialize().hex(), "%064x" % info.tree[(mh, pk)]] for mh, pk in zip(info.message_hashes, info.public_keys)]}


def case_objects(case):
    keys = {}
    return signature_of(case["dividend"], keys), [signature_of(d, keys) for d in case["divisors"]]


def outcome(fn):
    """("ok", [records]) or ("error", type name, text) of a call that returns a list of Signatures"""
    try:
        out = fn()
    except Exception as e:
        return ("error", type(e).__name__, str(e))
    return ("ok", [record_of(s) for s in out])


def expected_of(case):
    return ("error", "Exception", case["error"]) if "error" in case else ("ok", [case["result"]])


def expected_scalars(pt_off, ent_off, ea, eb):
    """(status bytes, scalars as ints, divisors with a quotient other than 1) of a call, in Python integers: the scalar of an
    accepted divisor is (-a_0 * pow(b_0, -1, n)) % n"""
    status, scalars, nonunit = [], [], 0
    for p in range(len(ent_off) - 1):
        lo, hi = ent_off[p], ent_off[p + 1]
        if lo == hi:
            status.append(0)
            scalars.append(1)
            continue
        a, b = [v % N for v in ea[lo:hi]], [v % N for v in eb[lo:hi]]
        if 0 in b:
            status.append(2)
            scalars.append(0)
        elif any(x * b[0] % N != a[0] * y % N for x, y in zip(a, b)):
            status.append(1)
            scalars.append(0)
        else:
            status.append(0)
            scalars.append((-a[0] * pow(b[0], -1, N)) % N)
            nonunit += scalars[-1] != N - 1
    return bytes(status), scalars, nonunit


class HostSigDivide:
    """a provider whose only offer is `sig_divide`, computed on the host with the mirror's curve arithmetic: results as
    bls_py._native_sigdiv.sig_divide gives them.  `calls` records (m, n_pts, n_ent) of every call."""

    def __init__(self):
        self.calls = []

    def sig_divide(self, pts, pt_off, ent_off, ea, eb):
        n_pts, m = len(pts) // 192, len(pt_off) - 1
        self.calls.append((m, n_pts, len(ea)))
        status, scalars, nonunit = expected_scalars(pt_off, ent_off, list(ea), list(eb))
        out, flag = [], []
        for j in range(m):
            acc, off, refused = None, False, False
            for p in range(pt_off[j], pt_off[j + 1]):
                A = H.g2_from_abi(pts[192 * p:192 * (p + 1)])
                off |= not H.on_curve(H.F2, A)
                refused |= status[p] != 0
                acc = H.jac_add(H.F2, acc, H.jac_mul(H.F2, H.aff_to_jac(H.F2, A), scalars[p]))
            if refused or off:
                out.append(bytes(192))
                flag.append(3 if refused else 2)
            else:
                A = H.jac_to_affine(H.F2, acc)
                out.append(H.g2_affine_bytes(A))
                flag.append(1 if A is None else 0)
        return b"".join(out), bytes(flag), status, b"".join(s.to_bytes(32, "big") for s in scalars), (int(nonunit != 0), nonunit)
