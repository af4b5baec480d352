"""Feldman share checks on the GPU (csrc/blsgpu_g1poly.hip) against the host loop, and the batched dealing:
  * one player checking its 100 incoming fragments at T = 67 (blsgpu_g1_poly_check_dev, device events; and
    Threshold.verify_secret_fragment_batch end to end, host clock);
  * the whole 100 x 100 x 67 matrix of a Joint-Feldman key generation, the same two ways, with 1 % of the fragments
    tampered -- every entry compared with the host loop Threshold.verify_secret_fragment, run in worker processes
    started before this process touches the GPU;
  * the host loop per fragment (one process);
  * PrivateKey.new_threshold_batch(67, 100, 100) against new_threshold(67, 100) one at a time;
  * a 1000-dealer x 1000-player matrix at T = 667 on the device (honest fragments for one player per dealer, the other
    fragments random: their expected status is 0).
usage: python3 tools/dkg_probe.py [out_dir (default profiles)] [repeats (default 5)] [host workers (default 15)]
Writes <out_dir>/dkg_probe.txt, stamped with the library's version string and a digest of libblsgpu.so."""
import hashlib
import multiprocessing as mp
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-bls_amd"))
N = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def _host_check(job):
    """worker: the host loop for a list of (fragment, player, dealer) against the dealers' commitments"""
    from bls_py import hostmath as H
    from bls_py.ec import AffinePoint
    from bls_py.fields import Fq
    from bls_py.threshold import Threshold
    T, commits, items = job
    C = {d: [AffinePoint._from(H.F1, a) for a in cs] for d, cs in commits.items()}
    return [Threshold.verify_secret_fragment(T, Fq(N, s), p, C[d]) for s, p, d in items]


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    workers = int(sys.argv[3]) if len(sys.argv) > 3 else 15
    pool = mp.get_context("spawn").Pool(workers)          # fresh interpreters, started before the GPU is opened

    import torch
    from bls_py import _native, backend, keys
    from bls_py import hostmath as H
    from bls_py.keys import PrivateKey
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

    def host_clock(fn, k):
        ts = []
        for _ in range(k):
            t0 = time.perf_counter()
            r = fn()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts), r

    def to_dev(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    with open(_native._LIB_PATH, "rb") as f:
        lib_digest = hashlib.sha256(f.read()).hexdigest()[:16]
    log("# dkg_probe: %s, libblsgpu.so sha256 %s, %s, %d repeats (median; device events unless marked host clock)"
        % (eng.version(), lib_digest, torch.cuda.get_device_name(0), reps))

    T, NP = 67, 100
    keys.RNG = random.Random(67100)
    deals = PrivateKey.new_threshold_batch(T, NP, NP)
    rnd = random.Random(1)
    tampered = set(rnd.sample(range(NP * NP), NP))
    frs, pls, cms, items = [], [], [], []
    for d, (_, C, frags) in enumerate(deals):
        for j in range(NP):
            k = d * NP + j
            f = frags[j] + 1 if k in tampered else frags[j]
            frs.append(f)
            pls.append(j + 1)
            cms.append(C)
            items.append((int(f), j + 1, d))
    commits = {d: [c._aff() for c in C] for d, (_, C, _) in enumerate(deals)}
    chunks = [items[i::workers] for i in range(workers)]
    host_async = pool.map_async(_host_check, [(T, commits, ch) for ch in chunks])
    t_host0 = time.perf_counter()

    commit = b"".join(H.g1_affine_bytes(c._aff()) for _, C, _ in deals for c in C)
    d_commit = to_dev(commit)

    def dev_case(sel):
        """device buffers of the fragments at positions sel (sorted by dealer already)"""
        poly = torch.tensor([items[k][2] for k in sel], dtype=torch.int32, device=dev)
        x = to_dev(b"".join(items[k][1].to_bytes(32, "big") for k in sel))
        s = to_dev(b"".join(items[k][0].to_bytes(32, "big") for k in sel))
        status = torch.zeros(len(sel), dtype=torch.uint8, device=dev)
        run = lambda: eng.g1_poly_check_dev(d_commit.data_ptr(), NP, T, poly.data_ptr(), x.data_ptr(), s.data_ptr(), len(sel),
                                            status.data_ptr(), None, st.cuda_stream)
        return run, status

    log("\n## device: blsgpu_g1_poly_check_dev (index scan + one sync, commitment preparation and subgroup checks, Horner)")
    log("%28s %10s %12s %14s" % ("case", "fragments", "ms", "fragments/s"))
    player7 = [d * NP + 6 for d in range(NP)]
    for name, sel in (("one player, 100 dealers", player7), ("100 x 100 matrix", list(range(NP * NP)))):
        run, status = dev_case(sel)
        run()
        st.synchronize()
        ms = statistics.median(timed(run) for _ in range(reps))
        ok = [b == 1 for b in bytes(status.cpu().numpy())]
        want = [k not in tampered for k in sel]
        log("%28s %10d %12.3f %14.3e   statuses as planted: %s" % (name, len(sel), ms, len(sel) / ms * 1e3, ok == want))

    log("\n## Python end to end: Threshold.verify_secret_fragment_batch (host clock)")
    t1, r1 = host_clock(lambda: Threshold.verify_secret_fragment_batch(T, [frs[k] for k in player7], [pls[k] for k in player7],
                                                                       [cms[k] for k in player7]), reps)
    log("one player, 100 fragments: %.2f ms" % (t1 * 1e3))
    t_all, got = host_clock(lambda: Threshold.verify_secret_fragment_batch(T, frs, pls, cms), 3)
    log("100 x 100 matrix (10 000 fragments): %.1f ms; False exactly at the %d tampered positions: %s"
        % (t_all * 1e3, len(tampered), [k for k, ok in enumerate(got) if not ok] == sorted(tampered)))

    log("\n## host loop: Threshold.verify_secret_fragment, T = 67 (hostmath)")
    t_one, _ = host_clock(lambda: Threshold.verify_secret_fragment(T, frs[5], pls[5], cms[5]), 5)
    log("one fragment, one process: %.1f ms -> 10 000 fragments %.0f s in one process" % (t_one * 1e3, t_one * 1e4))
    host = [None] * len(items)
    for i, res in enumerate(host_async.get()):
        host[i::workers] = res
    t_host = time.perf_counter() - t_host0
    log("all 10 000 in %d worker processes: %.1f s wall; agree with the batch on every entry: %s"
        % (workers, t_host, host == got))
    log("speed-up of the batch (end to end) over the one-process host loop: %.0fx" % (t_one * 1e4 / t_all))
    pool.close()
    pool.join()

    log("\n## dealing: PrivateKey.new_threshold_batch(67, 100, 100) vs new_threshold(67, 100) one at a time (host clock)")
    keys.RNG = random.Random(5)
    tb, _ = host_clock(lambda: PrivateKey.new_threshold_batch(T, NP, NP), 3)
    keys.RNG = random.Random(5)
    ts, _ = host_clock(lambda: PrivateKey.new_threshold(T, NP), 5)
    log("batch of 100 dealers: %.1f ms; one new_threshold: %.1f ms -> 100 of them %.1f s; speed-up %.0fx"
        % (tb * 1e3, ts * 1e3, ts * 100, ts * 100 / tb))

    log("\n## larger: 1000 dealers x 1000 players, T = 667 (device; honest fragments for player 7 of every dealer, the rest random)")
    T2, NP2 = 667, 1000
    r2 = random.Random(2)
    coeffs = [[r2.randrange(1, N) for _ in range(T2)] for _ in range(NP2)]
    aff, _ = eng.g1_mul_gen(b"".join(c.to_bytes(32, "big") for cs in coeffs for c in cs), ser=False)
    d_commit2 = to_dev(aff)
    honest = []
    for cs in coeffs:
        v = 0
        for c in reversed(cs):
            v = (v * 7 + c) % N
        honest.append(v)
    poly = torch.arange(NP2, dtype=torch.int32, device=dev).repeat_interleave(NP2)
    x = to_dev(b"".join((j + 1).to_bytes(32, "big") for _ in range(NP2) for j in range(NP2)))
    sb = bytearray(os.urandom(32 * NP2 * NP2))
    for d in range(NP2):
        k = d * NP2 + 6
        sb[32 * k:32 * (k + 1)] = honest[d].to_bytes(32, "big")
    s = to_dev(sb)
    status = torch.zeros(NP2 * NP2, dtype=torch.uint8, device=dev)
    run = lambda: eng.g1_poly_check_dev(d_commit2.data_ptr(), NP2, T2, poly.data_ptr(), x.data_ptr(), s.data_ptr(), NP2 * NP2,
                                        status.data_ptr(), None, st.cuda_stream)
    ms = timed(run)
    got2 = status.cpu().numpy().reshape(NP2, NP2)
    ok = bool((got2[:, 6] == 1).all()) and int((got2 == 1).sum()) == NP2 and int((got2 == 2).sum()) == 0
    log("1 000 000 fragments: %.1f ms (one run) = %.3e fragments/s; 1 exactly at the honest entries: %s" % (ms, 1e6 / ms * 1e3, ok))

    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "dkg_probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
