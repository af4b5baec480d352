"""Randomized batch verification (BLS.verify_batch_randomized) against BLS.verify_batch on the same inputs, and the subgroup
membership kernels (csrc/blsgpu_subgroup.hip):
  * 32 768 single-key signatures over distinct messages, and the same with one forgery (the combined check fails and
    every signature takes the exact path: the shape where the randomized form loses);
  * 32 768 signatures over 64 messages (committee shape);
  * 4 096 mixed aggregates (1 - 4 signatures each; every other aggregate over one shared message, secure aggregation);
  * G1 / G2 membership of 65 536 points (device events on the _dev forms, and the host-buffer forms end to end).
For each batch: end to end (host clock) and the part spent inside the provider's device entries (host clock around each
call: copies, launches and the wait for the result), median of the repeats.
usage: python3 tools/rlc_probe.py [out_dir (default profiles)] [repeats (default 3)]
Writes <out_dir>/rlc_probe.txt, stamped with the library's version string and a digest of libblsgpu.so."""
import hashlib
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-bls_amd"))
N = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


class Timed:
    """the HIP provider with every entry timed (host clock; the entries return host bytes, so each call includes its wait)"""

    def __init__(self, inner):
        self.inner = inner
        self.spent = 0.0
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self.inner, name)

        def call(*a, **k):
            t0 = time.perf_counter()
            r = fn(*a, **k)
            dt = time.perf_counter() - t0
            self.spent += dt
            self.calls.append((name, dt))
            return r
        return call


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    import torch
    from bls_py import _native, backend
    from bls_py import hostmath as H
    from bls_py.bls import BLS
    from bls_py.keys import PrivateKey

    eng = _native.engine(0)
    timed = Timed(backend.HipProvider())
    backend.use(timed)
    dev = torch.device("cuda", 0)
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    with open(_native._LIB_PATH, "rb") as f:
        lib_digest = hashlib.sha256(f.read()).hexdigest()[:16]
    log("# rlc_probe: %s, libblsgpu.so sha256 %s, %s, %d repeats (median)" % (eng.version(), lib_digest, torch.cuda.get_device_name(0), reps))

    def sks(tag, n):
        return [PrivateKey(int.from_bytes(hashlib.sha256(b"%s%d" % (tag, i)).digest(), "big") % (N - 1) + 1) for i in range(n)]

    def run(name, batch):
        for fn in (BLS.verify_batch, BLS.verify_batch_randomized):      # warm-up: the workspaces grow once
            fn(batch)
        rows = {}
        for label, fn in (("verify_batch", BLS.verify_batch), ("randomized", BLS.verify_batch_randomized)):
            tot, inside, res = [], [], None
            for _ in range(reps):
                timed.spent, timed.calls = 0.0, []
                t0 = time.perf_counter()
                res = fn(batch)
                tot.append(time.perf_counter() - t0)
                inside.append(timed.spent)
            rows[label] = (statistics.median(tot) * 1e3, statistics.median(inside) * 1e3, res, [c for c, _ in timed.calls])
        same = rows["verify_batch"][2] == rows["randomized"][2]
        log("%-44s %14s %14s   %s" % (name, "end to end ms", "in device ms", "device calls"))
        for label, (t, d, _, calls) in rows.items():
            log("  %-42s %14.1f %14.1f   %s" % (label, t, d, " ".join(calls)))
        log("  speed-up end to end %.2fx, in device calls %.2fx; same answers: %s; valid: %d of %d"
            % (rows["verify_batch"][0] / rows["randomized"][0], rows["verify_batch"][1] / rows["randomized"][1], same,
               sum(rows["randomized"][2]), len(batch)))

    n = 32768
    keys = sks(b"rlc-a", n)
    batch = PrivateKey.sign_batch(keys, [b"m%d" % i for i in range(n)])
    run("32768 single-key signatures, distinct messages", batch)
    batch[5] = keys[5].sign(b"forged")
    batch[5].set_aggregation_info(batch[6].aggregation_info)
    run("the same with one forgery (combined check fails)", batch)
    run("32768 signatures over 64 messages", PrivateKey.sign_batch(keys, [b"slot %d" % (i % 64) for i in range(n)]))
    ks, signers, msgs = sks(b"rlc-c", 4), [], []
    for a in range(4096):
        k = 1 + a % 4
        signers += ks[:k]
        msgs += [b"shared %d" % a] * k if a % 2 else [b"agg %d-%d" % (a, j) for j in range(k)]
    flat, mixed, pos = PrivateKey.sign_batch(signers, msgs), [], 0
    for a in range(4096):
        k = 1 + a % 4
        mixed.append(BLS.aggregate_sigs(flat[pos:pos + k]))
        pos += k
    run("4096 mixed aggregates (1-4 signatures)", mixed)

    # membership of 65 536 points: the fixture-free mix of subgroup points and random curve points
    rng = random.Random(1)
    m = 65536
    for g, psz, dev_fn, host_fn in (("g1", 96, eng.g1_subgroup_dev, eng.g1_subgroup), ("g2", 192, eng.g2_subgroup_dev, eng.g2_subgroup)):
        base = []
        for i in range(64):
            if g == "g1":
                A = H.jac_to_affine(H.F1, H.jac_mul(H.F1, H.aff_to_jac(H.F1, H.G1_GEN), rng.randrange(1, N))) if i % 2 else None
                while A is None:
                    try:
                        x = rng.randrange(H.Q)
                        A = (x, H.y_for_x(H.F1, x)[0])
                    except Exception:
                        A = None
                base.append(H.g1_affine_bytes(A))
            else:
                A = H.jac_to_affine(H.F2, H.jac_mul(H.F2, H.aff_to_jac(H.F2, H.G2_GEN), rng.randrange(1, N))) if i % 2 else None
                while A is None:
                    try:
                        x = (rng.randrange(H.Q), rng.randrange(H.Q))
                        A = (x, H.y_for_x(H.F2, x)[0])
                    except Exception:
                        A = None
                base.append(H.g2_affine_bytes(A))
        buf = b"".join(base[i % 64] for i in range(m))
        d_pts = torch.frombuffer(bytearray(buf), dtype=torch.uint8).to(dev)
        d_st = torch.zeros(m, dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream(dev)
        ev = []
        for _ in range(reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            dev_fn(d_pts.data_ptr(), m, d_st.data_ptr(), st.cuda_stream)
            b.record(st)
            b.synchronize()
            ev.append(a.elapsed_time(b))
        hc = []
        for _ in range(reps):
            t0 = time.perf_counter()
            out = host_fn(buf)
            hc.append(time.perf_counter() - t0)
        ok = out == bytes(1 if i % 2 else 2 for i in range(m)) and bytes(d_st.cpu().tolist()) == out
        d_ms = statistics.median(ev[1:])
        log("%s membership, %d points: device %.3f ms (%.1f M points/s), host buffers end to end %.2f ms; statuses as built: %s"
            % (g.upper(), m, d_ms, m / d_ms / 1e3, statistics.median(hc) * 1e3, ok))

    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "rlc_probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
