"""Batched Signature.divide_by (csrc/blsgpu_sigdiv.hip, blsgpu_sig_divide_dev), medians of 3 calls after one warm-up call.
Cases, the first two once with unit quotients (the plain path) and once with the quotients of a secure merge (the scalar path):
  (a) 10 000 dividends x 3 divisors x 4 entries;
  (b) one dividend with one divisor of 100 000 entries;
  (c) Signature.divide_by_batch end to end (wall clock) on 256 aggregates of 4 leaves, 3 of them divided out, against the loop.
(a) and (b) time blsgpu_sig_divide_dev (device events around the call, its synchronisation included) and, on the scalars it
wrote, blsgpu_g2_msm_ranges_dev alone -- so the share of the new kernels is visible -- and the host loop's arithmetic (one
pow(b, n - 2, n) per entry, one G2 multiplication and addition per divisor, as the mirror's divide_by does them) on a SAMPLE,
stated as SCALED to the case.
Every step is a child process under its own time limit; the first step that fails or runs out of time ends the probe.
usage: python3 tools/sigdiv_probe.py [out_dir (default profiles)]      writes <out_dir>/sigdiv_probe.txt"""
import os
import random
import statistics
import struct
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-bls_amd"))
N = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
REPS = 3
STEPS = (("a-unit", 240), ("a-secure", 240), ("b-unit", 240), ("b-secure", 240), ("c-python", 420))
SAMPLE = 8


def spread(ts):
    return "%9.3f  (min %.3f, max %.3f)" % (statistics.median(ts), min(ts), max(ts))


def device_case(label, m, divisors, entries, unit):
    import torch
    from bls_py import _native
    from bls_py import _native_msmr as R
    from bls_py import _native_sigdiv as S
    from bls_py import hostmath as H
    eng = _native.engine(0)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    rnd = random.Random(label)
    n_pts, n_ent = m * (1 + divisors), m * divisors * entries
    pts = eng.hash_to_g2(rnd.randbytes(32 * n_pts))
    pt_off = [j * (1 + divisors) for j in range(m + 1)]
    ent_off, ea, eb = [0], bytearray(), bytearray()
    for p in range(n_pts):
        if p % (1 + divisors):
            q = 1 if unit else rnd.randrange(2, N)
            for _ in range(entries):
                b = rnd.randrange(1, N)
                ea += (q * b % N).to_bytes(32, "big")
                eb += b.to_bytes(32, "big")
        ent_off.append(len(ea) // 32)
    up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    words = lambda v: struct.pack("<%dI" % len(v), *v)
    d_p, d_po, d_eo, d_a, d_b = up(pts), up(words(pt_off)), up(words(ent_off)), up(ea), up(eb)
    d_out, d_flag, d_st, d_sc = (torch.empty(s, dtype=torch.uint8, device=dev) for s in (192 * m, m, n_pts, 32 * n_pts))
    d_out2, d_flag2 = torch.empty(192 * m, dtype=torch.uint8, device=dev), torch.empty(m, dtype=torch.uint8, device=dev)
    d_rg = up(words([v for j in range(m) for v in (pt_off[j], pt_off[j + 1])]))
    stats = []

    def divide():
        stats.append(S.sig_divide_dev(eng, d_p.data_ptr(), n_pts, d_po.data_ptr(), m, d_eo.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), n_ent,
                                      d_out.data_ptr(), d_flag.data_ptr(), d_st.data_ptr(), d_sc.data_ptr(), st.cuda_stream))

    def sums_alone():
        R.g2_msm_ranges_dev(eng, d_p.data_ptr(), d_sc.data_ptr(), n_pts, d_rg.data_ptr(), m, d_out2.data_ptr(), d_flag2.data_ptr(), st.cuda_stream)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        return a.elapsed_time(b)

    out = []
    for fn in (divide, sums_alone):
        timed(fn)
        out.append([timed(fn) for _ in range(REPS)])
    same = bool(torch.equal(d_out, d_out2)) and int(d_st.max()) == 0
    # the host loop's arithmetic on a sample of divisors
    J = [H.aff_to_jac(H.F2, H.g2_from_abi(pts[192 * p:192 * (p + 1)])) for p in range(1, 1 + min(SAMPLE, divisors * m))]
    per_entry = min(entries, 64)
    t0 = time.perf_counter()
    acc = None
    for P in J:
        for e in range(per_entry):
            b = int.from_bytes(eb[32 * e:32 * e + 32], "big")
            q = int.from_bytes(ea[32 * e:32 * e + 32], "big") * pow(b, N - 2, N) % N
        acc = H.jac_add(H.F2, acc, H.jac_mul(H.F2, P, (-q) % N))
    host = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    for _ in range(len(J) * per_entry):
        pow(b, N - 2, N)
    pows = (time.perf_counter() - t0) * 1e3
    per_pow, per_div = pows / (len(J) * per_entry), (host - pows) / len(J)
    scaled = per_pow * n_ent + per_div * m * divisors
    return ["%s %d dividends x %d divisors x %d entries, %s quotients: path %d, %d non-unit" % ((label, m, divisors, entries, "unit" if unit else "secure") + stats[-1]),
            "    sig_divide_dev %s ms   g2_msm_ranges_dev alone on the same scalars %s ms   same bytes: %s" % (spread(out[0]), spread(out[1]), same),
            "    host loop's arithmetic, sample of %d divisors x %d entries SCALED: %.1f ms (%.4f ms per pow, %.3f ms per G2 multiplication and addition)"
            % (len(J), per_entry, scaled, per_pow, per_div)]


def python_case():
    from bls_py.bls import BLS
    from bls_py.keys import PrivateKey
    from bls_py.signature import Signature
    m, leaves = 256, 4
    sks = [PrivateKey.from_seed(b"sigdiv probe %d" % i) for i in range(m * leaves)]
    sigs = PrivateKey.sign_batch(sks, [b"message %d" % i for i in range(m * leaves)])
    dividends = [BLS.aggregate_sigs(sigs[leaves * j:leaves * (j + 1)]) for j in range(m)]
    lists = [sigs[leaves * j:leaves * j + 3] for j in range(m)]
    res = {}

    def wall(fn, key):
        t = time.perf_counter()
        res[key] = fn()
        return (time.perf_counter() - t) * 1e3
    batch = lambda: Signature.divide_by_batch(dividends, lists)
    sample = 16
    loop = lambda: [d.divide_by(ds) for d, ds in zip(dividends[:sample], lists[:sample])]
    wall(batch, "batch")
    tb = [wall(batch, "batch") for _ in range(REPS)]
    tl = [wall(loop, "loop") for _ in range(REPS)]
    same = [s.serialize() for s in res["batch"][:sample]] == [s.serialize() for s in res["loop"]]
    return ["(c) Signature.divide_by_batch end to end, %d aggregates of %d leaves, 3 divided out (unit quotients), wall clock" % (m, leaves),
            "    batch %s ms   loop of divide_by on %d of them SCALED to %d: %.1f ms   same signatures: %s"
            % (spread(tb), sample, m, statistics.median(tl) * m / sample, same)]


def step(name):
    if name == "c-python":
        return python_case()
    label, kind = name.split("-")
    shape = (10000, 3, 4) if label == "a" else (1, 1, 100000)
    return device_case("(%s)" % label, *shape, kind == "unit")


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        print("\n".join(step(sys.argv[2])), flush=True)
        return 0
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
    lines = ["# sigdiv_probe: medians of %d calls after 1 warm-up call (median, min, max); every step a process of its own" % REPS]
    rc = 0
    for name, limit in STEPS:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            lines.append("%s: no result within %d s; the probe ends here" % (name, limit))
            rc = 1
            break
        if r.returncode != 0:
            lines.append("%s: failed with status %d; the probe ends here\n%s" % (name, r.returncode, r.stderr[-2000:]))
            rc = 1
            break
        lines.append(r.stdout.rstrip())
    print("\n".join(lines), flush=True)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "sigdiv_probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
