"""Point range sums and the folded batch verification (csrc/blsgpu_pscan.hip), medians of 3 calls after one warm-up call:
  * blsgpu_g1_range_sums_dev / blsgpu_g2_range_sums_dev over equal-size ranges of 64 points against the plain group sums
    blsgpu_g1_msm_dev / blsgpu_g2_msm_dev(scalars = NULL, k = 64) of the same points, at 65 536 and 2^20 points (device events; the
    bytes compared);
  * 32 768 signatures over 64 messages and over 32 768 distinct messages, each with no forgery, one forgery and 1 % forgeries:
    blsgpu_verify_find_folded against -- in the same run, on the same inputs (sorted by message), alternating --
    blsgpu_verify_find and the device calls BLS.verify_batch_randomized makes (the two subgroup checks, hash to G2 of the distinct
    hashes, the G2 sum with the weights, the weighted keys summed per message, one multi-pairing of messages + 1 pairs; on a
    failure the n exact two-pair pairings of BLS.verify_batch as well).  Host-buffer forms, wall clock.  `stats` printed for each.
usage: python3 tools/fold_probe.py [out_dir (default profiles)] [signatures (default 32768)]
Writes <out_dir>/fold_probe.txt, stamped with the library's version string and a digest of libblsgpu.so."""
import hashlib
import os
import random
import statistics
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-bls_amd"))
N = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
REPS = 3


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 32768

    import torch
    from bls_py import _native
    from bls_py import _native_find as F
    from bls_py import _native_ranges as R
    from bls_py import hostmath as H

    eng = _native.Engine(0)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
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

    def wall(fn):
        t = time.perf_counter()
        fn()
        return (time.perf_counter() - t) * 1e3

    def spread(ts):
        return "%9.3f  (min %.3f, max %.3f)" % (statistics.median(ts), min(ts), max(ts))

    def to_dev(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    with open(_native._LIB_PATH, "rb") as f:
        lib_digest = hashlib.sha256(f.read()).hexdigest()[:16]
    log("# fold_probe: %s, libblsgpu.so sha256 %s, %s, medians of %d calls after 1 warm-up call (median, min, max)"
        % (eng.version(), lib_digest, torch.cuda.get_device_name(0), REPS))

    rnd = random.Random(65536)
    K = 64
    log("\n## sums over equal-size ranges of %d points, device events, ms" % K)
    for deg, psz in ((1, 96), (2, 192)):
        for m in (65536, 1 << 20):
            if deg == 1:
                pts = bytearray()
                for lo in range(0, m, 1 << 18):
                    pts += eng.g1_mul_gen(b"".join(rnd.randrange(1, N).to_bytes(32, "big") for _ in range(min(1 << 18, m - lo))), ser=False)[0]
            else:
                pts = eng.hash_to_g2(rnd.randbytes(32 * m))
            groups = m // K
            d_p = to_dev(pts)
            d_r = to_dev(struct.pack("<%dI" % (2 * groups), *[v for j in range(groups) for v in (j * K, (j + 1) * K)]))
            d_a = torch.empty(psz * groups, dtype=torch.uint8, device=dev)
            d_b = torch.empty(psz * groups, dtype=torch.uint8, device=dev)
            d_f = torch.empty(groups, dtype=torch.uint8, device=dev)
            sums_dev = R.g1_range_sums_dev if deg == 1 else R.g2_range_sums_dev
            msm = eng.lib.blsgpu_g1_msm_dev if deg == 1 else eng.lib.blsgpu_g2_msm_dev

            def f_ranges():
                sums_dev(eng, d_p.data_ptr(), m, d_r.data_ptr(), groups, d_a.data_ptr(), d_f.data_ptr(), st.cuda_stream)

            def f_msm():
                eng._check(msm(eng.h, d_p.data_ptr(), None, K, groups, d_b.data_ptr(), None, st.cuda_stream), "msm_dev")
            timed(f_ranges)
            timed(f_msm)
            ts, tm = [], []
            for _ in range(REPS):
                ts.append(timed(f_ranges))
                tm.append(timed(f_msm))
            log("G%d %8d points   range_sums_dev %s   msm_dev(NULL, k = %d) %s   ranges / msm %.3f   same bytes: %s"
                % (deg, m, spread(ts), K, spread(tm), statistics.median(ts) / statistics.median(tm), bool(torch.equal(d_a, d_b))))
            del d_p, d_r, d_a, d_b, d_f

    sks = [rnd.randrange(1, N) for _ in range(n)]
    skb = b"".join(s.to_bytes(32, "big") for s in sks)
    keys = eng.g1_mul_gen(skb, ser=False)[0]
    idx = list(range(n))
    weights = [rnd.getrandbits(64) or 1 for _ in range(n)]
    neg_g1 = H.g1_affine_bytes((H.G1_GEN[0], -H.G1_GEN[1] % H.Q))
    one = bytes(47) + b"\x01" + bytes(528)
    for n_msgs in (64, n):
        log("\n## %d signatures over %d messages, sorted by message, host-buffer calls, wall clock, ms" % (n, n_msgs))
        table = b"".join(hashlib.sha256(b"fold probe %d" % i).digest() for i in range(n_msgs))
        midx = [i * n_msgs // n for i in range(n)]
        per_item = b"".join(table[32 * j:32 * (j + 1)] for j in midx)
        good = eng.sign(skb, per_item, ser=False)[0]
        wrong = eng.sign(skb[32:] + skb[:32], per_item, ser=False)[0]        # signed by the next key
        for name, bad in (("no forgery", []), ("one forgery", [n // 3]), ("1 % forgeries", list(range(7, n, 100)))):
            sig = bytearray(good)
            for i in bad:
                sig[192 * i:192 * (i + 1)] = wrong[192 * i:192 * (i + 1)]
            sig = bytes(sig)
            expect = bytearray(b"\x01" * n)
            for i in bad:
                expect[i] = 0
            res = {}

            def f_fold():
                res["fold"] = R.verify_find_folded(eng, sig, keys, idx, table, midx, weights)

            def f_find():
                res["find"] = F.verify_find(eng, sig, keys, idx, table, midx, weights)

            def f_rand():
                eng.g2_subgroup(sig)
                eng.g1_subgroup(keys)
                hm = eng.hash_to_g2(table)
                S, _ = eng.g2_msm(sig, weights, n, 1)
                P, _ = eng.g1_msm(keys, weights, 1, n)
                if n_msgs != n:
                    P = b"".join(eng.g1_msm(P[96 * lo:96 * hi], None, hi - lo, 1)[0]
                                 for lo, hi in ((midx.index(j), n - midx[::-1].index(j)) for j in range(n_msgs)))
                ok = eng.pairing_multi(neg_g1 + P, S + hm, n_msgs + 1) == one
                res["rand"] = ok
                if not ok:
                    hi = b"".join(hm[192 * j:192 * (j + 1)] for j in midx)
                    g1 = b"".join(neg_g1 + keys[96 * i:96 * (i + 1)] for i in range(n))
                    g2 = b"".join(sig[192 * i:192 * (i + 1)] + hi[192 * i:192 * (i + 1)] for i in range(n))
                    eng.pairing_multi_batch(g1, g2, 2, n)
            f_fold(), f_find(), f_rand()
            tf, tp, tr = [], [], []
            for _ in range(REPS):
                tf.append(wall(f_fold))
                tp.append(wall(f_find))
                tr.append(wall(f_rand))
            log("\n### %s" % name)
            for label, ts, key in (("blsgpu_verify_find_folded", tf, "fold"), ("blsgpu_verify_find       ", tp, "find")):
                status, stats = res[key]
                log("%s %s   rounds %d, node tests %d, pairs %d; status as planted: %s"
                    % (label, spread(ts), stats[0], stats[1], stats[2], status == bytes(expect)))
            log("the calls of verify_batch_randomized (+ exact on failure) %s   combined check passed: %s; folded / find %.3f, folded / randomized %.3f"
                % (spread(tr), res["rand"], statistics.median(tf) / statistics.median(tp), statistics.median(tf) / statistics.median(tr)))

    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "fold_probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
