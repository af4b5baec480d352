"""Ragged multi-scalar sums (csrc/blsgpu_msmr.hip), medians of 3 calls after one warm-up call, _dev forms, device events, all in
one run.  For G1 and G2:
  (a) 1 range of 1024 points + 1024 ranges of 1 point: blsgpu_g?_msm_ranges_dev against the padded
      blsgpu_g?_msm_dev(k = 1024, groups = 1025) and against the per-length-class calls bls.py's _g1_group_sums makes
      (msm_dev(k = 1024, groups = 1) + msm_dev(k = 1, groups = 1024));
  (b) 10 000 ranges of 67 points (the C4 batch shape) against msm_dev(k = 67, groups = 10 000);
  (c) 65 536 ranges of 1 point against msm_dev(k = 1, groups = 65 536).
Then BLS.verify end to end (wall clock) on an aggregate of shape (a) -- one message with 1024 signers, 1024 messages with one --
as bls.py does it (padded key groups) and with the key sums from one ragged call handed to verify_pipeline(keys_affine=...).
usage: python3 tools/msm_ranges_probe.py [out_dir (default profiles)]
Writes <out_dir>/msm_ranges_probe.txt, stamped with the library's version string and a digest of libblsgpu.so.  Under
BLSGPU_LIBRARY=.../libblsgpu_msmru.so (make libblsgpu_msmru.so: k_smul_seg with the wavefront-uniform trip count) it measures
that library and writes <out_dir>/msm_ranges_probe_msmru.txt; the two files of one session are compared in DESIGN.md 2w."""
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

    import torch
    from bls_py import _native
    from bls_py import _native_msmr as R

    eng = _native.engine(0)
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

    def spread(ts):
        return "%9.3f  (min %.3f, max %.3f)" % (statistics.median(ts), min(ts), max(ts))

    def to_dev(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    def measure(fns):
        for f in fns:
            timed(f)
        ts = [[] for _ in fns]
        for _ in range(REPS):
            for t, f in zip(ts, fns):
                t.append(timed(f))
        return ts

    lib_path = os.environ.get("BLSGPU_LIBRARY", _native._LIB_PATH)
    with open(lib_path, "rb") as f:
        lib_digest = hashlib.sha256(f.read()).hexdigest()[:16]
    log("# msm_ranges_probe: %s, " % os.path.basename(lib_path) + "%s sha256 %s, %s, medians of %d calls after 1 warm-up call (median, min, max), device events, ms"
        % (eng.version(), lib_digest, torch.cuda.get_device_name(0), REPS))

    rnd = random.Random(1024)
    TOP = 10000 * 67
    for deg, psz in ((1, 96), (2, 192)):
        if deg == 1:
            pts = bytearray()
            for lo in range(0, TOP, 1 << 18):
                pts += eng.g1_mul_gen(b"".join(rnd.randrange(1, N).to_bytes(32, "big") for _ in range(min(1 << 18, TOP - lo))), ser=False)[0]
            pts = bytes(pts)
        else:
            pts = eng.hash_to_g2(rnd.randbytes(32 * TOP))
        sc = rnd.randbytes(32 * TOP)
        d_p, d_s = to_dev(pts), to_dev(sc)
        ranges_dev = R.g1_msm_ranges_dev if deg == 1 else R.g2_msm_ranges_dev
        msm = eng.lib.blsgpu_g1_msm_dev if deg == 1 else eng.lib.blsgpu_g2_msm_dev

        def ragged(n, ranges, d_out, d_flag, d_pts=d_p, d_sc=d_s):
            d_r = to_dev(struct.pack("<%dI" % (2 * len(ranges)), *[v for r in ranges for v in r]))
            return lambda: ranges_dev(eng, d_pts.data_ptr(), d_sc.data_ptr(), n, d_r.data_ptr(), len(ranges), d_out.data_ptr(), d_flag.data_ptr(),
                                      st.cuda_stream)

        def uniform(d_pts, d_sc, k, groups, d_out, d_inf):
            return lambda: eng._check(msm(eng.h, d_pts, d_sc, k, groups, d_out, d_inf, st.cuda_stream), "msm_dev")

        log("\n## G%d" % deg)
        # (a) the skewed mix
        L = 1024
        n = 2 * L
        ranges = [(0, L)] + [(L + i, L + i + 1) for i in range(L)]
        m = len(ranges)
        d_a, d_fa = torch.empty(psz * m, dtype=torch.uint8, device=dev), torch.empty(m, dtype=torch.uint8, device=dev)
        d_b, d_fb = torch.empty(psz * m, dtype=torch.uint8, device=dev), torch.empty(m, dtype=torch.uint8, device=dev)
        d_c, d_fc = torch.empty(psz * m, dtype=torch.uint8, device=dev), torch.empty(m, dtype=torch.uint8, device=dev)
        pad_p = bytearray(psz * L * m)
        pad_s = bytearray(32 * L * m)
        pad_p[:psz * L], pad_s[:32 * L] = pts[:psz * L], sc[:32 * L]
        for i in range(L):
            pad_p[psz * L * (i + 1):psz * L * (i + 1) + psz] = pts[psz * (L + i):psz * (L + i + 1)]
            pad_s[32 * L * (i + 1):32 * L * (i + 1) + 32] = sc[32 * (L + i):32 * (L + i + 1)]
        d_pp, d_ps = to_dev(pad_p), to_dev(pad_s)
        del pad_p, pad_s
        f_rag = ragged(n, ranges, d_a, d_fa)
        f_pad = uniform(d_pp.data_ptr(), d_ps.data_ptr(), L, m, d_b.data_ptr(), d_fb.data_ptr())
        c1 = uniform(d_p.data_ptr(), d_s.data_ptr(), L, 1, d_c.data_ptr(), d_fc.data_ptr())
        c2 = uniform(d_p.data_ptr() + psz * L, d_s.data_ptr() + 32 * L, 1, L, d_c.data_ptr() + psz, d_fc.data_ptr() + 1)

        def f_cls():
            c1()
            c2()
        tr, tp, tc = measure([f_rag, f_pad, f_cls])
        log("(a) 1 x %d + %d x 1   msm_ranges_dev %s   padded msm_dev(k = %d, groups = %d) %s   per-length-class calls (2) %s"
            % (L, L, spread(tr), L, m, spread(tp), spread(tc)))
        log("    ragged / padded %.3f   ragged / per-length-class %.3f   same bytes: padded %s, per-class %s"
            % (statistics.median(tr) / statistics.median(tp), statistics.median(tr) / statistics.median(tc),
               bool(torch.equal(d_a, d_b)), bool(torch.equal(d_a, d_c))))
        del d_pp, d_ps, d_a, d_b, d_c
        # (b) and (c): uniform shapes, recorded only
        for label, k, groups in (("(b)", 67, 10000), ("(c)", 1, 65536)):
            n = k * groups
            ranges = [(j * k, (j + 1) * k) for j in range(groups)]
            d_a, d_fa = torch.empty(psz * groups, dtype=torch.uint8, device=dev), torch.empty(groups, dtype=torch.uint8, device=dev)
            d_b, d_fb = torch.empty(psz * groups, dtype=torch.uint8, device=dev), torch.empty(groups, dtype=torch.uint8, device=dev)
            tr, tu = measure([ragged(n, ranges, d_a, d_fa), uniform(d_p.data_ptr(), d_s.data_ptr(), k, groups, d_b.data_ptr(), d_fb.data_ptr())])
            log("%s %d x %d   msm_ranges_dev %s   msm_dev(k = %d, groups = %d) %s   ragged / uniform %.3f   same bytes: %s"
                % (label, groups, k, spread(tr), k, groups, spread(tu), statistics.median(tr) / statistics.median(tu), bool(torch.equal(d_a, d_b))))
            del d_a, d_b
        del d_p, d_s

    # BLS.verify end to end on shape (a): as bls.py does it (the key groups padded to the longest for verify_pipeline) against
    # the same verification with the per-message key sums from ONE ragged call handed to verify_pipeline(keys_affine=...)
    from bls_py import backend
    from bls_py import hostmath as H
    from bls_py.bls import BLS, _jac_g1_bytes
    from bls_py.bls12381 import n as ORDER
    from bls_py.ec import default_ec, generator_Fq
    from bls_py.fields import Fq12
    from bls_py.keys import PrivateKey
    backend.use(None)
    L = 1024
    sks = [PrivateKey.from_seed(b"msm ranges probe %d" % i) for i in range(2 * L)]
    agg = BLS.aggregate_sigs(PrivateKey.sign_batch(sks, [b"shared"] * L + [b"own %d" % i for i in range(L)]))
    neg_g1 = H.g1_affine_bytes((generator_Fq() * (ORDER - 1))._aff())
    one = Fq12.one(default_ec.q).serialize()

    def verify_ragged(signature):
        info = signature.aggregation_info
        by_message = {}
        for mh, pk in zip(info.message_hashes, info.public_keys):
            by_message.setdefault(mh, []).append(pk)
        pts, sc, ranges, lo = bytearray(), bytearray(), [], 0
        for mh, keys in by_message.items():
            uniq = list(set(keys))
            for pk in uniq:
                pts += _jac_g1_bytes(pk.value)
                sc += (int(info.tree[(mh, pk)]) % ORDER).to_bytes(32, "big")
            ranges.append((lo, lo + len(uniq)))
            lo += len(uniq)
        keys, _ = R.g1_msm_ranges(eng, bytes(pts), bytes(sc), ranges)
        sig = H.g2_affine_bytes(signature.value.to_affine()._aff())
        return backend.get().verify_pipeline(neg_g1, sig, b"".join(by_message), len(by_message), keys_affine=keys) == one

    res = {}

    def wall(fn, key):
        t = time.perf_counter()
        res[key] = fn(agg)
        return (time.perf_counter() - t) * 1e3
    wall(verify_ragged, "ragged"), wall(BLS.verify, "padded")
    tr, tp = [], []
    for _ in range(REPS):
        tr.append(wall(verify_ragged, "ragged"))
        tp.append(wall(BLS.verify, "padded"))
    log("\n## BLS.verify end to end, one message with %d signers + %d messages with one, wall clock, ms" % (L, L))
    log("key sums from one ragged call + verify_pipeline(keys_affine) %s   BLS.verify (padded key groups) %s   ragged / padded %.3f   verdicts: %s, %s"
        % (spread(tr), spread(tp), statistics.median(tr) / statistics.median(tp), res["ragged"], res["padded"]))

    os.makedirs(out_dir, exist_ok=True)
    stem = os.path.splitext(os.path.basename(lib_path))[0]
    name = "msm_ranges_probe.txt" if stem == "libblsgpu" else "msm_ranges_probe_%s.txt" % stem.replace("libblsgpu_", "")
    with open(os.path.join(out_dir, name), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
