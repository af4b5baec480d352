"""The ragged secure aggregation (blsgpu_hash_pks_ranges_dev, blsgpu_aggregate_pub_keys_secure_ranges_dev,
blsgpu_aggregate_sigs_secure_ranges_dev) against the loop it would replace: one uniform _dev call per size class over the same
buffers (groups of one length lie side by side, so both read the lists as they are).  Medians of 3 calls after one warm-up
call, _dev forms, device events, all in one run:
  (a) 1000 groups of 2 .. 201 keys (five of each): 200 size classes;
  (b) 10 000 groups of 100: one size class;
  (c) one group of 1024 + 1024 groups of one.
Every group has as many exponents (points, signatures) as keys; the device hashes the keys in both paths.  The bytes of the two
paths are compared.  No ratio is fixed in advance: whatever comes out is recorded, a loss included; nothing is routed by default.
usage: python3 tools/secure_ranges_probe.py [out_dir (default profiles)]
Writes <out_dir>/secure_ranges_probe.txt, stamped with the library's version string and a digest of libblsgpu.so."""
import hashlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-bls_amd"))
REPS = 3


def shapes():
    """(label, [(length, how many)] in the order the groups lie in the lists)"""
    return [("(a) 1000 groups of 2 .. 201 keys", [(v, 5) for v in range(2, 202)]),
            ("(b) 10000 groups of 100", [(100, 10000)]),
            ("(c) 1 group of 1024 + 1024 groups of 1", [(1024, 1), (1, 1024)])]


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")

    import torch
    from bls_py import _native
    from bls_py import _native_secranges as S

    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    q = st.cuda_stream
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        return a.elapsed_time(b)

    def spread(ts):
        return "%9.3f  (min %.3f, max %.3f)" % (statistics.median(ts), min(ts), max(ts))

    def measure(fns):
        for f in fns:
            timed(f)
        ts = [[] for _ in fns]
        for _ in range(REPS):
            for t, f in zip(ts, fns):
                t.append(timed(f))
        return ts

    with open(os.path.join(ROOT, "tests", "golden", "pairs_seed1_g1.bin"), "rb") as f:
        g1 = f.read()
    with open(os.path.join(ROOT, "tests", "golden", "pairs_seed1_g2.bin"), "rb") as f:
        g2 = f.read()
    top = max(sum(v * k for v, k in cls) for _, cls in shapes())
    reps = -(-top // 1025)
    d_g1 = torch.frombuffer(bytearray((g1 * reps)[:96 * top]), dtype=torch.uint8).to(dev)     # the 1025 seeded points, over and over
    d_g2 = torch.frombuffer(bytearray((g2 * reps)[:192 * top]), dtype=torch.uint8).to(dev)
    gen = torch.Generator(device="cpu")
    gen.manual_seed(20240611)
    d_ser = torch.randint(0, 256, (48 * top,), dtype=torch.uint8, generator=gen).to(dev)      # hash_pks hashes bytes: they need not be points

    eng = _native.Engine(0)
    with open(os.environ.get("BLSGPU_LIBRARY", _native._LIB_PATH), "rb") as f:
        lib_digest = hashlib.sha256(f.read()).hexdigest()[:16]
    log("# secure_ranges_probe: %s sha256 %s, %s, medians of %d calls after 1 warm-up call (median, min, max), device events, ms"
        % (eng.version(), lib_digest, torch.cuda.get_device_name(0), REPS))

    for label, classes in shapes():
        off = [0]
        for v, k in classes:
            for _ in range(k):
                off.append(off[-1] + v)
        n, m = off[-1], len(off) - 1
        d_off = torch.tensor(off, dtype=torch.int64).to(torch.int32).to(dev)
        log("\n## %s: %d keys, %d groups, %d size classes" % (label, n, m, len(classes)))

        def buffers(item):
            return [torch.zeros(item * count, dtype=torch.uint8, device=dev) for count in (n if item == 32 else m, m) for _ in range(2)]

        # the exponents: m = k per group
        ta, tb, _, _ = buffers(32)

        def hash_ragged():
            S.hash_pks_ranges_dev(eng, d_ser.data_ptr(), n, d_off.data_ptr(), d_off.data_ptr(), n, m, None, ta.data_ptr(), None, q)

        def hash_classes():
            at = 0
            for v, k in classes:
                eng.hash_pks_dev(d_ser.data_ptr() + 48 * at, v, k, None, v, tb.data_ptr() + 32 * at, None, q)
                at += v * k
        ts = measure([hash_classes, hash_ragged])
        log("hash_pks: per-class loop of hash_pks_dev (%d calls)            %s" % (len(classes), spread(ts[0])))
        log("hash_pks: hash_pks_ranges_dev                                  %s   ragged / per-class %.3f   same bytes: %s"
            % (spread(ts[1]), statistics.median(ts[1]) / statistics.median(ts[0]), bool(torch.equal(ta, tb))))
        del ta, tb

        for name, psz, d_pts in (("pub_keys", 96, d_g1), ("sigs", 192, d_g2)):
            oa, ob, fa, fb = buffers(psz)

            def agg_ragged():
                if psz == 96:
                    S.aggregate_pub_keys_secure_ranges_dev(eng, d_pts.data_ptr(), d_ser.data_ptr(), n, d_off.data_ptr(), m, None, oa.data_ptr(),
                                                           fa.data_ptr(), q)
                else:
                    S.aggregate_sigs_secure_ranges_dev(eng, d_pts.data_ptr(), n, d_off.data_ptr(), d_ser.data_ptr(), n, d_off.data_ptr(), m, None,
                                                       oa.data_ptr(), fa.data_ptr(), q)

            def agg_classes():
                at, res = 0, 0
                for v, k in classes:
                    if psz == 96:
                        eng.aggregate_pub_keys_secure_dev(d_pts.data_ptr() + psz * at, d_ser.data_ptr() + 48 * at, None, v, k, ob.data_ptr() + psz * res,
                                                          fb.data_ptr() + res, q)
                    else:
                        eng.aggregate_sigs_secure_dev(d_pts.data_ptr() + psz * at, v, d_ser.data_ptr() + 48 * at, v, None, k, ob.data_ptr() + psz * res,
                                                      fb.data_ptr() + res, q)
                    at, res = at + v * k, res + k
            ts = measure([agg_classes, agg_ragged])
            same = bool(torch.equal(oa, ob)) and bool(torch.equal(fa, fb))
            log("%-8s: per-class loop of the uniform _dev call (%d calls)       %s" % (name, len(classes), spread(ts[0])))
            log("%-8s: the _ranges_dev call                                     %s   ragged / per-class %.3f   same bytes: %s"
                % (name, spread(ts[1]), statistics.median(ts[1]) / statistics.median(ts[0]), same))
            del oa, ob, fa, fb

    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "secure_ranges_probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
