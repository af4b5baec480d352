"""Short-scalar multiplication and bisecting batch verification (csrc/blsgpu_smul64.hip, csrc/blsgpu_batchfind.hip), medians
of 3 calls after one warm-up call:
  * blsgpu_g1_mul_short_dev / blsgpu_g2_mul_short_dev against blsgpu_g1_msm_dev / blsgpu_g2_msm_dev(k = 1) on the same weights
    zero-extended to 32 bytes, at 4096, 65 536 and 2^20 points (device events; the bytes compared);
  * blsgpu_verify_find on 32 768 signatures over distinct messages with no forgery, one forgery and 1 % forgeries, against
    -- in the same run, on the same inputs, alternating -- the device calls BLS.verify_batch_randomized makes (the two subgroup
    checks, hash to G2, the G2 sum with the weights, the weighted keys, one multi-pairing of n + 1 pairs; on a failure the n
    exact two-pair pairings of BLS.verify_batch as well) and the exact calls of BLS.verify_batch alone (hash to G2 and n
    two-pair pairings).  Host-buffer forms on both sides, wall clock: uploads and read-backs are part of every figure.
usage: python3 tools/batch_find_probe.py [out_dir (default profiles)] [signatures (default 32768)]
Writes <out_dir>/batch_find_probe.txt, stamped with the library's version string and a digest of libblsgpu.so."""
import hashlib
import os
import random
import statistics
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
    log("# batch_find_probe: %s, libblsgpu.so sha256 %s, %s, medians of %d calls after 1 warm-up call (median, min, max)"
        % (eng.version(), lib_digest, torch.cuda.get_device_name(0), REPS))

    rnd = random.Random(32768)
    log("\n## multiplication by 64-bit weights, device events, ms")
    for deg, psz in ((1, 96), (2, 192)):
        for m in (4096, 65536, 1 << 20):
            if deg == 1:
                pts = bytearray()
                for lo in range(0, m, 1 << 18):
                    pts += eng.g1_mul_gen(b"".join(rnd.randrange(1, N).to_bytes(32, "big") for _ in range(min(1 << 18, m - lo))), ser=False)[0]
            else:
                pts = eng.hash_to_g2(rnd.randbytes(32 * m))
            w = rnd.randbytes(8 * m)
            w32 = b"".join(bytes(24) + w[8 * i:8 * (i + 1)] for i in range(m))
            d_p, d_w, d_w32 = to_dev(pts), to_dev(w), to_dev(w32)
            d_a = torch.empty(psz * m, dtype=torch.uint8, device=dev)
            d_b = torch.empty(psz * m, dtype=torch.uint8, device=dev)
            short_dev = F.g1_mul_short_dev if deg == 1 else F.g2_mul_short_dev
            msm = eng.lib.blsgpu_g1_msm_dev if deg == 1 else eng.lib.blsgpu_g2_msm_dev

            def f_short():
                short_dev(eng, d_p.data_ptr(), d_w.data_ptr(), m, d_a.data_ptr(), None, st.cuda_stream)

            def f_msm():
                eng._check(msm(eng.h, d_p.data_ptr(), d_w32.data_ptr(), 1, m, d_b.data_ptr(), None, st.cuda_stream), "msm_dev")
            timed(f_short)
            timed(f_msm)
            ts, tm = [], []
            for _ in range(REPS):
                ts.append(timed(f_short))
                tm.append(timed(f_msm))
            same = bool(torch.equal(d_a, d_b))
            log("G%d %8d points   mul_short_dev %s   msm_dev(k = 1) %s   short / msm %.3f   same bytes: %s"
                % (deg, m, spread(ts), spread(tm), statistics.median(ts) / statistics.median(tm), same))
            del d_p, d_w, d_w32, d_a, d_b

    log("\n## %d signatures over distinct messages, host-buffer calls, wall clock, ms" % n)
    sks = [rnd.randrange(1, N) for _ in range(n)]
    skb = b"".join(s.to_bytes(32, "big") for s in sks)
    hashes = b"".join(hashlib.sha256(b"batch find probe %d" % i).digest() for i in range(n))
    keys = eng.g1_mul_gen(skb, ser=False)[0]
    good = eng.sign(skb, hashes, ser=False)[0]
    wrong = eng.sign(skb[32:] + skb[:32], hashes, ser=False)[0]            # signed by the next key
    idx = list(range(n))
    weights = [rnd.getrandbits(64) or 1 for _ in range(n)]
    neg_g1 = H.g1_affine_bytes((H.G1_GEN[0], -H.G1_GEN[1] % H.Q))
    one = bytes(47) + b"\x01" + bytes(528)

    for name, bad in (("no forgery", []), ("one forgery", [n // 3]), ("1 % forgeries", list(range(7, n, 100)))):
        sig = bytearray(good)
        for i in bad:
            sig[192 * i:192 * (i + 1)] = wrong[192 * i:192 * (i + 1)]
        sig = bytes(sig)
        expect = bytearray(b"\x01" * n)
        for i in bad:
            expect[i] = 0
        res = {}

        def f_find():
            res["find"] = F.verify_find(eng, sig, keys, idx, hashes, idx, weights)

        def f_exact():
            hm = eng.hash_to_g2(hashes)
            g1 = b"".join(neg_g1 + keys[96 * i:96 * (i + 1)] for i in range(n))
            g2 = b"".join(sig[192 * i:192 * (i + 1)] + hm[192 * i:192 * (i + 1)] for i in range(n))
            out = eng.pairing_multi_batch(g1, g2, 2, n)
            res["exact"] = bytes(int(out[576 * i:576 * (i + 1)] == one) for i in range(n))

        def f_rand():
            eng.g2_subgroup(sig)
            eng.g1_subgroup(keys)
            hm = eng.hash_to_g2(hashes)
            S, _ = eng.g2_msm(sig, weights, n, 1)
            P, _ = eng.g1_msm(keys, weights, 1, n)
            ok = eng.pairing_multi(neg_g1 + P, S + hm, n + 1) == one
            res["rand"] = ok
            if not ok:
                f_exact()
        f_find(), f_rand(), f_exact()
        tf, tr, te = [], [], []
        for _ in range(REPS):
            tf.append(wall(f_find))
            tr.append(wall(f_rand))
            te.append(wall(f_exact))
        status, stats = res["find"]
        log("\n### %s" % name)
        log("blsgpu_verify_find                                   %s   rounds %d, node tests %d, pairs %d; status as planted: %s"
            % (spread(tf), stats[0], stats[1], stats[2], status == bytes(expect)))
        log("the calls of verify_batch_randomized (+ exact on failure) %s   combined check passed: %s; find / randomized: %.3f"
            % (spread(tr), res["rand"], statistics.median(tf) / statistics.median(tr)))
        log("the calls of verify_batch (hash, %d two-pair pairings) %s   status as planted: %s; find / exact: %.3f"
            % (n, spread(te), res["exact"] == bytes(expect), statistics.median(tf) / statistics.median(te)))

    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "batch_find_probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
