"""Batched threshold recovery (csrc/blsgpu_lagrange.hip) by stage, against the G2 sum it feeds and against the host loop:
  * blsgpu_lagrange_at_zero_dev alone at 10 000 x 67, 1000 x 667 and 1 x 67 (device events);
  * blsgpu_threshold_combine_dev at 10 000 x 67 -- every group a different seeded 67-subset of players 1..100 of
    tests/golden/threshold.json's sharing -- next to its two stages timed separately in the same run, alternating: the
    Lagrange kernel and blsgpu_g2_msm_dev on the same shape with the coefficients precomputed (the sum is the code of the
    previous revision: the yardstick);
  * blsgpu_fr_interpolate_at_zero_dev at 10 000 x 67;
  * Threshold.aggregate_unit_sigs_batch end to end in Python (host clock: conversions, upload, device, download) against
    the host loop [Threshold.aggregate_unit_sigs(...)] on 100 of the groups, SCALED to 10 000; and
    Threshold.lagrange_coeffs_at_zero on this host, per group.
Every combined signature is compared with the fixture's.
usage: python3 tools/lagrange_probe.py [out_dir (default profiles)] [repeats (default 7)]
Writes <out_dir>/lagrange_probe.txt, stamped with the library's version string and a digest of libblsgpu.so."""
import hashlib
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-bls_amd"))
N = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7

    import torch
    from bls_py import _native, backend, util
    from bls_py import hostmath as H
    from bls_py.ec import JacobianPoint
    from bls_py.signature import Signature
    from bls_py.threshold import Threshold

    eng = _native.Engine(0)
    backend.use(backend.HipProvider())
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

    def be32(vs):
        return b"".join(v.to_bytes(32, "big") for v in vs)

    with open(_native._LIB_PATH, "rb") as f:
        lib_digest = hashlib.sha256(f.read()).hexdigest()[:16]
    log("# lagrange_probe: %s, libblsgpu.so sha256 %s, %s, %d repeats after 2 warm-up calls (median, min, max; device events "
        "unless marked host clock)" % (eng.version(), lib_digest, torch.cuda.get_device_name(0), reps))

    with open(os.path.join(ROOT, "tests", "golden", "threshold.json")) as f:
        th = json.load(f)["67_of_100"]
    poly = [int(c, 16) for c in th["poly"]]

    def share(x):
        acc = 0
        for c in reversed(poly):
            acc = (acc * x + c) % N
        return acc
    hm = eng.hash_to_g2(util.hash256(bytes.fromhex(th["msg"])))
    unit, _ = eng.g2_msm(hm * 100, [share(x) for x in range(1, 101)], 1, 100)
    unit = [unit[192 * i:192 * (i + 1)] for i in range(100)]
    gold = bytes.fromhex(th["combined_affine"])
    rnd = random.Random(10000)
    groups, k = 10000, 67
    subsets = [rnd.sample(range(1, 101), k) for _ in range(groups)]
    sig_bytes = b"".join(unit[p - 1] for S in subsets for p in S)
    x_bytes = be32([p for S in subsets for p in S])

    # ---- the Lagrange kernel alone -----------------------------------------------------------------------------------
    log("\n## device: blsgpu_lagrange_at_zero_dev (k_lagrange: one point per lane, a Fermat inversion per lane and one per group)")
    log("%16s %10s %36s %14s" % ("groups x k", "points", "ms", "groups/s"))
    shapes = [(10000, 67, x_bytes), (1000, 667, be32([p for _ in range(1000) for p in rnd.sample(range(1, 1001), 667)])),
              (1, 67, x_bytes[:32 * 67])]
    for g, kk, xb in shapes:
        d_x = to_dev(xb)
        d_co = torch.empty(32 * g * kk, dtype=torch.uint8, device=dev)
        d_st = torch.empty(g, dtype=torch.uint8, device=dev)
        run = lambda: eng.lagrange_at_zero_dev(d_x.data_ptr(), kk, g, d_co.data_ptr(), d_st.data_ptr(), st.cuda_stream)  # noqa: E731
        for _ in range(2):
            timed(run)
        ts = [timed(run) for _ in range(reps)]
        ok = int(d_st.sum().item()) == g
        log("%16s %10d %36s %14.4g   all status 1: %s" % ("%d x %d" % (g, kk), g * kk, spread(ts), g / statistics.median(ts) * 1e3, ok))

    # ---- the combine and its two stages --------------------------------------------------------------------------------
    log("\n## device: blsgpu_threshold_combine_dev at 10 000 x 67 and its stages, alternating in one loop")
    d_sig, d_x = to_dev(sig_bytes), to_dev(x_bytes)
    d_co = torch.empty(32 * groups * k, dtype=torch.uint8, device=dev)
    d_st = torch.empty(groups, dtype=torch.uint8, device=dev)
    d_out = torch.empty(192 * groups, dtype=torch.uint8, device=dev)
    d_out2 = torch.empty(192 * groups, dtype=torch.uint8, device=dev)
    d_inf = torch.empty(groups, dtype=torch.uint8, device=dev)
    f_lag = lambda: eng.lagrange_at_zero_dev(d_x.data_ptr(), k, groups, d_co.data_ptr(), d_st.data_ptr(), st.cuda_stream)  # noqa: E731
    f_sum = lambda: eng._check(eng.lib.blsgpu_g2_msm_dev(eng.h, d_sig.data_ptr(), d_co.data_ptr(), k, groups, d_out2.data_ptr(),  # noqa: E731
                                                         d_inf.data_ptr(), st.cuda_stream), "blsgpu_g2_msm_dev")
    f_all = lambda: eng.threshold_combine_dev(d_sig.data_ptr(), d_x.data_ptr(), k, groups, d_out.data_ptr(), d_inf.data_ptr(),  # noqa: E731
                                              d_st.data_ptr(), st.cuda_stream)
    for _ in range(2):
        for f in (f_lag, f_sum, f_all):
            timed(f)
    t = {"lag": [], "sum": [], "all": []}
    for _ in range(reps):
        t["lag"].append(timed(f_lag))
        t["sum"].append(timed(f_sum))
        t["all"].append(timed(f_all))
    out = bytes(d_out.cpu().numpy())
    good = all(out[192 * g:192 * (g + 1)] == gold for g in range(groups))
    same = bool((d_out == d_out2).all().item())
    log("k_lagrange (coefficients of 10 000 different subsets)      %s ms" % spread(t["lag"]))
    log("blsgpu_g2_msm_dev, precomputed coefficients (the yardstick) %s ms" % spread(t["sum"]))
    log("blsgpu_threshold_combine_dev (both, no host round trip)     %s ms" % spread(t["all"]))
    log("Lagrange stage / G2 sum: %.3f; every group equals the fixture's combined signature: %s; combine == sum of its stages' "
        "output: %s; status sum %d" % (statistics.median(t["lag"]) / statistics.median(t["sum"]), good, same, int(d_st.sum().item())))

    d_y = to_dev(be32([rnd.randrange(N) for _ in range(groups * k)]))
    d_v = torch.empty(32 * groups, dtype=torch.uint8, device=dev)
    f_dot = lambda: eng.fr_interpolate_at_zero_dev(d_x.data_ptr(), d_y.data_ptr(), k, groups, d_v.data_ptr(), d_st.data_ptr(), st.cuda_stream)  # noqa: E731
    for _ in range(2):
        timed(f_dot)
    log("blsgpu_fr_interpolate_at_zero_dev (k_lagrange + k_fr_dot)    %s ms" % spread([timed(f_dot) for _ in range(reps)]))

    # ---- Python end to end against the host loop -----------------------------------------------------------------------
    log("\n## Python end to end: Threshold.aggregate_unit_sigs_batch, 10 000 groups of 67 (host clock)")
    objs = [Signature.from_g2(JacobianPoint._from(H.F2, H.aff_to_jac(H.F2, H.g2_from_abi(u)))) for u in unit]
    sig_groups = [[objs[p - 1] for p in S] for S in subsets]
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        res = Threshold.aggregate_unit_sigs_batch(sig_groups, subsets, 67)
        ts.append(time.perf_counter() - t0)
    want = Signature.from_g2(JacobianPoint._from(H.F2, H.aff_to_jac(H.F2, H.g2_from_abi(gold)))).serialize()
    log("batch: %.2f s (min %.2f, max %.2f over 3 calls; %.3f ms per group -- with the byte strings of the "
        "670 000 listed points joined on the host); all equal the fixture: %s" % (statistics.median(ts), min(ts), max(ts), statistics.median(ts) / groups * 1e3,
                                                 all(r.serialize() == want for r in res[::97])))
    t0 = time.perf_counter()
    loop = [Threshold.aggregate_unit_sigs(s, p, 67) for s, p in zip(sig_groups[:100], subsets[:100])]
    t_loop = time.perf_counter() - t0
    log("host loop [aggregate_unit_sigs(...)] on 100 groups: %.2f s = %.1f ms per group; SCALED to 10 000 groups: %.0f s "
        "(one device sum per group, one host Lagrange evaluation per group); equal to the batch: %s"
        % (t_loop, t_loop * 10, t_loop * 100, all(a.serialize() == b.serialize() for a, b in zip(loop, res))))
    ts = []
    for S in subsets[:20]:
        t0 = time.perf_counter()
        Threshold.lagrange_coeffs_at_zero(S)
        ts.append(time.perf_counter() - t0)
    log("Threshold.lagrange_coeffs_at_zero(67 players) on this host: %.1f ms per group (median of 20; min %.1f, max %.1f) -> "
        "%.0f s for 10 000 groups" % (statistics.median(ts) * 1e3, min(ts) * 1e3, max(ts) * 1e3, statistics.median(ts) * groups))
    t0 = time.perf_counter()
    co = Threshold.lagrange_coeffs_at_zero_batch(subsets)
    t_b = time.perf_counter() - t0
    log("Threshold.lagrange_coeffs_at_zero_batch(10 000 groups): %.2f s (host clock, Fq objects built for 670 000 coefficients); "
        "group 0 equals the single call: %s" % (t_b, co[0] == Threshold.lagrange_coeffs_at_zero(subsets[0])))

    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "lagrange_probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
