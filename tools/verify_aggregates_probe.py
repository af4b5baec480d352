"""blsgpu_verify_aggregates against the calls of today's BLS.verify_batch on the same inputs, in one run.  Medians of 3 calls
after one warm-up call:
  (a) 32 768 plain single-key signatures over distinct messages;
  (b) 32 768 single-key signatures over 64 messages;
  (c) 1000 aggregates of 2 .. 201 messages (five of each), one key per message;
  (d) the skewed aggregate of tools/msm_ranges_probe.py: one message with 1024 keys plus 1024 messages with one key.
Per shape: BLS.verify_batch(fused=False) end to end and the part of it spent inside the provider's device calls (hash_to_g2,
g1_msm, pairing_multi_batch), the host-buffer call blsgpu_verify_aggregates alone on the arguments verify_batch(fused=True)
assembles, and BLS.verify_batch(fused=True) end to end.  The products of the fused call are held against those the default path's
pairing_multi_batch calls returned, byte for byte.  The call inherits two known losses -- the serial chain of the ragged sums on a
long group and the ragged multi-pairing's loss on one long range: shapes (c) and (d) are there to show them.  No ratio is fixed in
advance; BLS.verify_batch stays unrouted, and whoever routes it quotes this file.
usage: python3 tools/verify_aggregates_probe.py [out_dir (default profiles)] [scale divisor (default 1: the shapes above)]
Writes <out_dir>/verify_aggregates_probe.txt, stamped with the library's version string and a digest of libblsgpu.so."""
import hashlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-bls_amd"))
REPS = 3


class Recording:
    """the installed provider with the time spent in, and the results of, its device calls"""

    def __init__(self, prov):
        self._prov, self.spent, self.pairings = prov, 0.0, []

    def __getattr__(self, name):
        fn = getattr(self._prov, name)
        if not callable(fn):
            return fn

        def call(*a, **k):
            t0 = time.perf_counter()
            out = fn(*a, **k)
            self.spent += time.perf_counter() - t0
            if name == "pairing_multi_batch":
                self.pairings.append((a[2], out))
            return out
        return call


def build(shape, scale):
    """the signatures of a shape, made with the library's own batch methods"""
    from bls_py.bls import BLS
    from bls_py.keys import PrivateKey
    n = max(8, 32768 // scale)
    if shape == "a":
        sks = [PrivateKey.from_seed(b"probe-a-%d" % (i % 256)) for i in range(256)]
        return PrivateKey.sign_batch([sks[i % 256] for i in range(n)], [b"message %d" % i for i in range(n)])
    if shape == "b":
        sks = [PrivateKey.from_seed(b"probe-b-%d" % (i % 256)) for i in range(256)]
        return PrivateKey.sign_batch([sks[i % 256] for i in range(n)], [b"shared %d" % (i % 64) for i in range(n)])
    if shape == "c":
        sks = [PrivateKey.from_seed(b"probe-c-%d" % i) for i in range(201)]
        out = []
        for k in range(2, 202, max(1, scale)):
            for r in range(5):
                out.append(BLS.aggregate_sigs(PrivateKey.sign_batch(sks[:k], [b"agg %d %d %d" % (k, r, i) for i in range(k)])))
        return out
    k = max(4, 1024 // scale)
    sks = [PrivateKey.from_seed(b"probe-d-%d" % i) for i in range(2 * k)]
    return [BLS.aggregate_sigs(PrivateKey.sign_batch(sks, [b"skewed shared"] * k + [b"skewed own %d" % i for i in range(k)]))]


def fused_arguments(signatures):
    """what BLS.verify_batch(fused=True) hands to the extension, captured from it"""
    from bls_py import backend
    from bls_py.bls import BLS
    real = backend.extension("verify_aggregates")
    seen = []

    class Capture:
        def __init__(self, prov):
            self._prov = prov

        def __getattr__(self, name):
            return getattr(self._prov, name)

        def verify_aggregates(self, *a, **k):
            seen.append(a)
            return real(*a, **k)
    prov = backend.get()
    backend.use(Capture(prov))
    try:
        results = BLS.verify_batch(signatures, fused=True)
    finally:
        backend.use(prov)
    return seen[0], results


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
    scale = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    from bls_py import _native, backend
    from bls_py.bls import BLS
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    def spread(ts):
        return "%10.2f ms  (min %.2f, max %.2f)" % (1e3 * statistics.median(ts), 1e3 * min(ts), 1e3 * max(ts))

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    lib = os.environ.get("BLSGPU_LIBRARY", os.path.join(ROOT, "python-bls_amd", "csrc", "libblsgpu.so"))
    with open(lib, "rb") as f:
        digest = hashlib.sha256(f.read()).hexdigest()[:16]
    log("verify_aggregates probe: %s, libblsgpu.so sha256 %s, scale 1/%d, medians of %d" % (_native.engine(0).version(), digest, scale, REPS))
    backend.use(None)
    prov = backend.get()
    fused = backend.extension("verify_aggregates")
    labels = {"a": "(a) single-key signatures over distinct messages", "b": "(b) single-key signatures over 64 messages",
              "c": "(c) aggregates of 2 .. 201 messages", "d": "(d) one message with many keys plus as many messages with one key"}
    for shape in "abcd":
        sigs = build(shape, scale)
        args, want = fused_arguments(sigs)                                   # (also the warm-up of the fused path)
        sizes = [len({mh for mh, _ in s.aggregation_info.tree}) + 1 for s in sigs]
        log("%s: %d signatures, %d pairs, %d keys, %d distinct messages" % (labels[shape], len(sigs), sum(sizes), len(args[2]) // 96,
                                                                          len(args[1]) // 32))
        rec = Recording(prov)
        backend.use(rec)
        try:
            assert BLS.verify_batch(sigs) == want                            # warm-up of the default path
            t_default, t_device = [], []
            for _ in range(REPS):
                rec.spent, rec.pairings = 0.0, []
                t, got = timed(lambda: BLS.verify_batch(sigs))
                assert got == want
                t_default.append(t)
                t_device.append(rec.spent)
        finally:
            backend.use(prov)
        status, gt = fused(*args, gt=True)
        assert [st == 1 for st in status] == want and all(want)
        # the same bytes: the default path's pairing calls hold the aggregates of one pair count in the order of the list
        at = {}
        by_size = {size: out for size, out in rec.pairings}
        for j, size in enumerate(sizes):
            i = at.get(size, 0)
            assert gt[576 * j:576 * (j + 1)] == by_size[size][576 * i:576 * (i + 1)], (shape, j)
            at[size] = i + 1
        t_call = [timed(lambda: fused(*args))[0] for _ in range(REPS)]
        t_fused = [timed(lambda: BLS.verify_batch(sigs, fused=True))[0] for _ in range(REPS)]
        log("  verify_batch(fused=False) end to end   %s" % spread(t_default))
        log("    of which inside the provider's calls  %s  (%d of them pairing calls)" % (spread(t_device), len(rec.pairings)))
        log("  blsgpu_verify_aggregates, host buffers  %s" % spread(t_call))
        log("  verify_batch(fused=True) end to end     %s" % spread(t_fused))
        log("  the fused products equal the default path's, byte for byte")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "verify_aggregates_probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
