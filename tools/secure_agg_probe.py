"""Secure aggregation with the hash_pks exponents on the device against the path it replaces, device-resident with device
events after warm-up, the forms alternating in one process per step on the same inputs:
  batch pub|sig|priv k groups   (n) blsgpu_aggregate_pub_keys_secure_dev / blsgpu_aggregate_sigs_secure_dev /
                                blsgpu_aggregate_priv_keys_secure_dev (with both key outputs): digests, exponents and sums in one
                                call, against (p) the path before it: the Python hash_pks loop (one hashlib call and one
                                big-integer % per exponent), timed by the wall clock on HOST_GROUPS groups and scaled, plus the
                                existing sum call -- blsgpu_g1_msm_dev / blsgpu_g2_msm_dev on exponents already on the device
                                (their upload is NOT counted), or for private keys the Python integers of
                                BLS.aggregate_priv_keys on the same sample.
  digest k groups               the 64-group rule: (dev) blsgpu_hash_pks_dev hashing the keys itself against (host) hashlib over
                                the groups by the wall clock plus blsgpu_hash_pks_dev with the digests handed in.
  single n                      ONE group of n public keys: the host's digest (wall clock) and (n)
                                blsgpu_aggregate_pub_keys_secure_dev with it handed in, against (p) the Python hash_pks loop on
                                HOST_OUTPUTS outputs, scaled, plus blsgpu_g1_msm_dev.
Each device time is reported as min and median of the repeats; outputs are compared in every step.  No ratio is required.

usage: python3 tools/secure_agg_probe.py [out_dir (default profiles)] [repeats (default 10)]
The driver makes no GPU call itself: every step is a child process of its own under `timeout`, and the first child that
fails ends the run.  Writes <out_dir>/secure_agg_probe.txt, stamped with the library's version string and a digest of
libblsgpu.so."""
import hashlib
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-bls_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from deal_probe import N_ORDER, _scalars, _setup  # noqa: E402
from keygen_probe import _alternate  # noqa: E402

BATCH = (100, 10000)                                                     # keys per group, groups
DIGEST_GROUPS = (64, 10000)
SINGLE = 1 << 20
HOST_GROUPS = 50
HOST_OUTPUTS = 20000
STEP_SECONDS = 420


def _line(name, t, count, unit):
    med = statistics.median(t)
    print("%-52s %10.3f %10.3f %14.3e %s/s" % (name, min(t), med, count / med * 1e3, unit), flush=True)


def _host_ts(ser, k, m):
    """util.hash_pks(m, keys) for the serialised keys of ONE group, as the Python loop computes it"""
    digest = hashlib.sha256(ser).digest()
    return [int.from_bytes(hashlib.sha256(i.to_bytes(4, "big") + digest).digest(), "big") % N_ORDER for i in range(m)]


def _keys(torch, eng, dev, st, seed, n):
    """n seeded public keys on the device: (affine bytes, serialised bytes)"""
    d_sk = _scalars(torch, torch.Generator().manual_seed(seed), n).to(dev)
    d_aff = torch.zeros(96 * n, dtype=torch.uint8, device=dev)
    d_ser = torch.zeros(48 * n, dtype=torch.uint8, device=dev)
    eng.g1_mul_gen_dev(d_sk.data_ptr(), n, d_aff.data_ptr(), d_ser.data_ptr(), st.cuda_stream)
    st.synchronize()
    return d_aff, d_ser


def step_batch(which, k, groups, reps):
    torch, eng, dev, st = _setup("secure aggregation (%s), %d groups of %d" % (which, groups, k), reps)
    s, n = st.cuda_stream, k * groups
    d_aff, d_ser = _keys(torch, eng, dev, st, 7 * k + groups, n)
    d_ts = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
    eng.hash_pks_dev(d_ser.data_ptr(), k, groups, None, k, d_ts.data_ptr(), None, s)
    if which == "pub":
        d_n, d_p = (torch.zeros(96 * groups, dtype=torch.uint8, device=dev) for _ in range(2))
        forms = (("n", lambda: eng.aggregate_pub_keys_secure_dev(d_aff.data_ptr(), d_ser.data_ptr(), None, k, groups, d_n.data_ptr(), None, s)),
                 ("p", lambda: eng._check(eng.lib.blsgpu_g1_msm_dev(eng.h, d_aff.data_ptr(), d_ts.data_ptr(), k, groups, d_p.data_ptr(), None, s),
                                          "blsgpu_g1_msm_dev")))
        names = {"n": "(n) aggregate_pub_keys_secure_dev", "p": "(p) g1_msm_dev, exponents on the device"}
    elif which == "sig":
        from bls_py import hostmath as H
        g2 = H.g2_affine_bytes(H.G2_GEN)
        d_g2 = torch.tensor(list(g2), dtype=torch.uint8, device=dev)
        d_sc = _scalars(torch, torch.Generator().manual_seed(n), n).to(dev)
        d_sigs = torch.zeros(192 * n, dtype=torch.uint8, device=dev)
        eng.g2_mul_secret_dev(d_g2.data_ptr(), 1, d_sc.data_ptr(), n, d_sigs.data_ptr(), None, None, s)
        d_n, d_p = (torch.zeros(192 * groups, dtype=torch.uint8, device=dev) for _ in range(2))
        forms = (("n", lambda: eng.aggregate_sigs_secure_dev(d_sigs.data_ptr(), k, d_ser.data_ptr(), k, None, groups, d_n.data_ptr(), None, s)),
                 ("p", lambda: eng._check(eng.lib.blsgpu_g2_msm_dev(eng.h, d_sigs.data_ptr(), d_ts.data_ptr(), k, groups, d_p.data_ptr(), None, s),
                                          "blsgpu_g2_msm_dev")))
        names = {"n": "(n) aggregate_sigs_secure_dev", "p": "(p) g2_msm_dev, exponents on the device"}
    else:
        sk = _scalars(torch, torch.Generator().manual_seed(n + 1), n)
        d_sk = sk.to(dev)
        d_n, d_a, d_s = (torch.zeros(w * groups, dtype=torch.uint8, device=dev) for w in (32, 96, 48))
        forms = (("n", lambda: eng.aggregate_priv_keys_secure_dev(d_sk.data_ptr(), d_ser.data_ptr(), None, k, groups, d_n.data_ptr(),
                                                                  d_a.data_ptr(), d_s.data_ptr(), s)),)
        names = {"n": "(n) aggregate_priv_keys_secure_dev, sums and keys"}
    t = _alternate(st, forms, reps)
    print("%-52s %10s %10s %14s" % ("path", "min", "median", "rate"))
    for key in names:
        _line(names[key], t[key], groups, "groups")
    # the Python loop the new call replaces, on a sample of the groups
    m = min(groups, HOST_GROUPS)
    ser = bytes(d_ser[:48 * k * m].cpu().tolist())
    t0 = time.perf_counter()
    host_ts = [_host_ts(ser[48 * k * g:48 * k * (g + 1)], k, k) for g in range(m)]
    wall = time.perf_counter() - t0
    print("(p) Python hash_pks loop on %d of the %d groups: %.3f ms per group by the wall clock -> %.1f ms for %d groups (scaled; the other %d NOT MEASURED)"
          % (m, groups, wall / m * 1e3, wall / m * groups * 1e3, groups, groups - m))
    dev_ts = bytes(d_ts[:32 * k * m].cpu().tolist())
    print("exponents of those equal the device's: %s" % (dev_ts == b"".join(v.to_bytes(32, "big") for g in host_ts for v in g)))
    new = statistics.median(t["n"])
    if which == "priv":
        raw = bytes(sk[:32 * k * m].tolist())
        ints = [int.from_bytes(raw[32 * i:32 * (i + 1)], "big") for i in range(k * m)]
        t0 = time.perf_counter()
        host = [sum(a * b for a, b in zip(ints[g * k:(g + 1) * k], host_ts[g])) % N_ORDER for g in range(m)]
        aff = [eng.g1_mul_gen(v.to_bytes(32, "big"), ser=False)[0] for v in host]          # one round trip per key, as get_public_key makes
        wall2 = time.perf_counter() - t0
        print("(p) Python integer sums and one g1_mul_gen per key on those groups: %.3f ms per group -> %.1f ms for %d groups (scaled)"
              % (wall2 / m * 1e3, wall2 / m * groups * 1e3, groups))
        print("sums of those equal the device's: %s, keys: %s"
              % (bytes(d_n[:32 * m].cpu().tolist()) == b"".join(v.to_bytes(32, "big") for v in host),
                 bytes(d_a[:96 * m].cpu().tolist()) == b"".join(aff)))
        old = (wall + wall2) / m * groups * 1e3
    else:
        print("outputs equal: %s" % bool(torch.equal(d_n, d_p)))
        old = wall / m * groups * 1e3 + statistics.median(t["p"])
    print("(p) / (n) = %.1f on medians, the Python parts scaled (recorded)" % (old / new), flush=True)
    eng.close()


def step_digest(k, groups, reps):
    torch, eng, dev, st = _setup("hash_pks, %d groups of %d: who computes the digests" % (groups, k), reps)
    s = st.cuda_stream
    _, d_ser = _keys(torch, eng, dev, st, k + groups, k * groups)
    ser = d_ser.cpu().numpy().tobytes()
    walls = []
    for _ in range(5):
        t0 = time.perf_counter()
        dg = b"".join(hashlib.sha256(ser[48 * k * g:48 * k * (g + 1)]).digest() for g in range(groups))
        walls.append((time.perf_counter() - t0) * 1e3)
    d_dg = torch.tensor(list(dg), dtype=torch.uint8, device=dev)
    d_a, d_b = (torch.zeros(32 * k * groups, dtype=torch.uint8, device=dev) for _ in range(2))
    d_odg = torch.zeros(32 * groups, dtype=torch.uint8, device=dev)
    forms = (("dev", lambda: eng.hash_pks_dev(d_ser.data_ptr(), k, groups, None, k, d_a.data_ptr(), d_odg.data_ptr(), s)),
             ("host", lambda: eng.hash_pks_dev(None, k, groups, d_dg.data_ptr(), k, d_b.data_ptr(), None, s)))
    t = _alternate(st, forms, reps)
    print("%-52s %10s %10s %14s" % ("path", "min", "median", "rate"))
    _line("(dev) hash_pks_dev, digests and exponents", t["dev"], groups, "groups")
    _line("(host) hash_pks_dev, digests handed in", t["host"], groups, "groups")
    print("(host) hashlib over the %d groups: min %.3f, median %.3f ms by the wall clock (the upload of %d bytes NOT MEASURED)"
          % (groups, min(walls), statistics.median(walls), 32 * groups))
    print("digests equal: %s, exponents equal: %s" % (d_odg.cpu().numpy().tobytes() == dg, bool(torch.equal(d_a, d_b))))
    print("(host: hashlib + call) / (dev) = %.2f on medians (recorded)"
          % ((statistics.median(walls) + statistics.median(t["host"])) / statistics.median(t["dev"])), flush=True)
    eng.close()


def step_single(n, reps):
    torch, eng, dev, st = _setup("aggregate_pub_keys(secure=True), ONE group of %d keys, the digest from the host" % n, reps)
    s = st.cuda_stream
    d_aff, d_ser = _keys(torch, eng, dev, st, n, n)
    ser = d_ser.cpu().numpy().tobytes()
    walls = []
    for _ in range(5):
        t0 = time.perf_counter()
        dg = hashlib.sha256(ser).digest()
        walls.append((time.perf_counter() - t0) * 1e3)
    d_dg = torch.tensor(list(dg), dtype=torch.uint8, device=dev)
    d_ts = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
    eng.hash_pks_dev(None, n, 1, d_dg.data_ptr(), n, d_ts.data_ptr(), None, s)
    d_n, d_p = (torch.zeros(96, dtype=torch.uint8, device=dev) for _ in range(2))
    forms = (("n", lambda: eng.aggregate_pub_keys_secure_dev(d_aff.data_ptr(), None, d_dg.data_ptr(), n, 1, d_n.data_ptr(), None, s)),
             ("p", lambda: eng._check(eng.lib.blsgpu_g1_msm_dev(eng.h, d_aff.data_ptr(), d_ts.data_ptr(), n, 1, d_p.data_ptr(), None, s),
                                      "blsgpu_g1_msm_dev")))
    t = _alternate(st, forms, reps)
    print("%-52s %10s %10s %14s" % ("path", "min", "median", "rate"))
    _line("(n) aggregate_pub_keys_secure_dev, digest handed in", t["n"], n, "keys")
    _line("(p) g1_msm_dev, exponents on the device", t["p"], n, "keys")
    print("host digest of %d bytes (both paths): min %.3f, median %.3f ms by the wall clock" % (len(ser), min(walls), statistics.median(walls)))
    m = min(n, HOST_OUTPUTS)
    t0 = time.perf_counter()
    host = [int.from_bytes(hashlib.sha256(i.to_bytes(4, "big") + dg).digest(), "big") % N_ORDER for i in range(m)]
    wall = time.perf_counter() - t0
    print("(p) Python hash_pks loop on %d of the %d outputs: %.3f us per output by the wall clock -> %.1f ms for all (scaled; the other %d NOT MEASURED)"
          % (m, n, wall / m * 1e6, wall / m * n * 1e3, n - m))
    print("exponents of those equal the device's: %s, sums equal: %s"
          % (bytes(d_ts[:32 * m].cpu().tolist()) == b"".join(v.to_bytes(32, "big") for v in host), bool(torch.equal(d_n, d_p))))
    print("(p) / (n) = %.1f on medians, the Python loop scaled, the host digest in both (recorded)"
          % ((statistics.median(walls) + wall / m * n * 1e3 + statistics.median(t["p"])) / (statistics.median(walls) + statistics.median(t["n"]))),
          flush=True)
    eng.close()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step-batch":
        step_batch(sys.argv[2], *(int(a) for a in sys.argv[3:6]))
        return 0
    if len(sys.argv) > 1 and sys.argv[1] == "--step-digest":
        step_digest(*(int(a) for a in sys.argv[2:5]))
        return 0
    if len(sys.argv) > 1 and sys.argv[1] == "--step-single":
        step_single(*(int(a) for a in sys.argv[2:4]))
        return 0
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
    reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 10
    lines = ["# secure_agg_probe: secure aggregation with the hash_pks exponents on the device against the Python loop and the existing "
             "sums, device-resident; one child process per step"]
    rc = 0
    steps = [("batch %s" % w, ["--step-batch", w, str(BATCH[0]), str(BATCH[1]), str(reps)]) for w in ("pub", "sig", "priv")]
    steps += [("digest %d" % g, ["--step-digest", str(BATCH[0]), str(g), str(reps)]) for g in DIGEST_GROUPS]
    steps.append(("single", ["--step-single", str(SINGLE), str(reps)]))
    for what, args in steps:
        p = subprocess.run(["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__)] + args,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        print(p.stdout, end="", flush=True)
        lines += ["", *p.stdout.rstrip("\n").split("\n")]
        if p.returncode != 0:
            rc = p.returncode
            lines.append("step %s ended with status %d: stopped here" % (what, rc))
            print(lines[-1], flush=True)
            break
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "secure_agg_probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
