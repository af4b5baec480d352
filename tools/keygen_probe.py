"""Public keys from private keys, timed device-resident with device events after warm-up (csrc/blsgpu_g1fix.hip), at 1, 4096,
65 536 and 2^20 scalars, the three paths alternating in one process per size on the same scalars:
  (s) blsgpu_g1_mul_gen_secret_dev: k_fix_mul_secret, 65 mixed additions on a schedule that does not depend on the scalar;
  (t) blsgpu_g1_mul_gen_dev: k_fix_mul, up to 32 mixed additions gathered by the scalar's 8-bit digits;
  (m) blsgpu_g1_msm_dev(k = 1, groups = n): the variable-base path (k_smul from 4096 sums).
Each is reported as min and median of the repeats; the outputs of the three are compared.
Required: (s) faster than (m) at 65 536 and 2^20 -- below that a G1 port of k_g2_smul would serve a caller better.
Recorded: (s) / (t), whatever it is.
A last step times blsgpu_hd_paths_secret_dev against blsgpu_hd_paths_dev(priv) at 65 536 paths of depth 4.

usage: python3 tools/keygen_probe.py [out_dir (default profiles)] [repeats (default 20)]
The driver makes no GPU call itself: every size is a child process of its own under `timeout`, and the first child that
fails ends the run.  Writes <out_dir>/keygen_probe.txt, stamped with the library's version string and a digest of
libblsgpu.so."""
import hashlib
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-bls_amd"))
SIZES = (1, 4096, 65536, 1 << 20)
HD_PATHS, HD_DEPTH = 65536, 4
STEP_SECONDS = 240


def _head(what, eng, reps):
    import torch
    from bls_py import _native
    with open(_native._LIB_PATH, "rb") as f:
        digest = hashlib.sha256(f.read()).hexdigest()[:16]
    print("## %s: %s, libblsgpu.so sha256 %s, %s, %d repeats after 3 warm-up rounds (ms, device events)"
          % (what, eng.version(), digest, torch.cuda.get_device_name(0), reps), flush=True)


def _timed(st, fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    fn()
    b.record(st)
    b.synchronize()
    return a.elapsed_time(b)


def _alternate(st, forms, reps):
    for _ in range(3):
        for _, fn in forms:
            _timed(st, fn)
    t = {k: [] for k, _ in forms}
    for _ in range(reps):
        for k, fn in forms:
            t[k].append(_timed(st, fn))
    return t


def step(n, reps):
    import torch
    from bls_py import _native
    eng = _native.Engine(0)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    _head("n = %d" % n, eng, reps)
    gen = torch.Generator().manual_seed(n)
    sk = torch.randint(0, 256, (n, 32), dtype=torch.uint8, generator=gen)
    sk[:, 0] &= 0x3F                                     # below 2^254 < n: what a private key is
    d_sk = sk.reshape(-1).to(dev)
    g1 = torch.tensor(list(bytes.fromhex(
        "17f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb"
        "08b3f481e3aaa0f1a09e30ed741d8ae4fcf5e095d5d00af600db18cb2c04b3edd03cc744a2888ae40caa232946c5e7e1")), dtype=torch.uint8)
    d_pts = g1.repeat(n).to(dev)                        # the generator, once per group of one point
    d_s, d_t, d_m = (torch.zeros(96 * n, dtype=torch.uint8, device=dev) for _ in range(3))
    d_inf = torch.zeros(n, dtype=torch.uint8, device=dev)
    s = st.cuda_stream
    forms = (("s", lambda: eng.g1_mul_gen_secret_dev(d_sk.data_ptr(), n, d_s.data_ptr(), None, s)),
             ("t", lambda: eng.g1_mul_gen_dev(d_sk.data_ptr(), n, d_t.data_ptr(), None, s)),
             ("m", lambda: eng._check(eng.lib.blsgpu_g1_msm_dev(eng.h, d_pts.data_ptr(), d_sk.data_ptr(), 1, n, d_m.data_ptr(),
                                                                 d_inf.data_ptr(), s), "g1_msm_dev")))
    t = _alternate(st, forms, reps)
    names = {"s": "(s) g1_mul_gen_secret_dev", "t": "(t) g1_mul_gen_dev", "m": "(m) g1_msm_dev(k=1)"}
    print("%-32s %10s %10s %14s" % ("path", "min", "median", "scalars/s"))
    for k, _ in forms:
        med = statistics.median(t[k])
        print("%-32s %10.3f %10.3f %14.3e" % (names[k], min(t[k]), med, n / med * 1e3))
    print("outputs equal: (s) == (t) %s, (s) == (m) %s" % (bool(torch.equal(d_s, d_t)), bool(torch.equal(d_s, d_m))))
    s_med, t_med, m_med = (statistics.median(t[k]) for k in "stm")
    print("(s) / (m) = %.3f on medians%s" % (s_med / m_med, (": required (s) faster than (m): %s" % ("met" if s_med < m_med else "MISSED"))
                                             if n >= 65536 else ""))
    print("(s) / (t) = %.3f on medians (recorded)" % (s_med / t_med), flush=True)
    eng.close()


def step_hd(reps):
    import torch
    from bls_py import _native
    eng = _native.Engine(0)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    n, depth = HD_PATHS, HD_DEPTH
    _head("%d private paths of depth %d" % (n, depth), eng, reps)
    gen = torch.Generator().manual_seed(7)
    chain = bytes(torch.randint(0, 256, (32,), dtype=torch.uint8, generator=gen).tolist())
    sk = bytes([0x21] + torch.randint(0, 256, (31,), dtype=torch.uint8, generator=gen).tolist())
    aff, _ = eng.g1_mul_gen(sk)
    d_par = torch.tensor(list(chain + aff + sk), dtype=torch.uint8, device=dev)
    d_idx = torch.randint(0, 1 << 32, (n * depth,), dtype=torch.int64, generator=gen).to(dev).to(torch.int32)
    widths = (32, 32, 96, 48, 4)
    o_s = [torch.zeros(w * n, dtype=torch.uint8, device=dev) for w in widths]
    o_p = [torch.zeros(w * n, dtype=torch.uint8, device=dev) for w in widths]
    s = st.cuda_stream
    forms = (("s", lambda: eng.hd_paths_secret_dev(d_par.data_ptr(), 1, None, d_idx.data_ptr(), depth, n, *[o.data_ptr() for o in o_s], s)),
             ("p", lambda: eng.hd_paths_dev(d_par.data_ptr(), 1, True, None, d_idx.data_ptr(), depth, n, *[o.data_ptr() for o in o_p], s)))
    t = _alternate(st, forms, reps)
    names = {"s": "(s) hd_paths_secret_dev", "p": "(p) hd_paths_dev(priv)"}
    print("%-32s %10s %10s %14s" % ("path", "min", "median", "paths/s"))
    for k, _ in forms:
        med = statistics.median(t[k])
        print("%-32s %10.3f %10.3f %14.3e" % (names[k], min(t[k]), med, n / med * 1e3))
    print("outputs equal: %s" % all(bool(torch.equal(a, b)) for a, b in zip(o_s, o_p)))
    print("(s) / (p) = %.3f on medians (recorded)" % (statistics.median(t["s"]) / statistics.median(t["p"])), flush=True)
    eng.close()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        step(int(sys.argv[2]), int(sys.argv[3]))
        return 0
    if len(sys.argv) > 1 and sys.argv[1] == "--step-hd":
        step_hd(int(sys.argv[2]))
        return 0
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
    reps = max(20, int(sys.argv[2])) if len(sys.argv) > 2 else 20
    lines = ["# keygen_probe: public keys from private keys, device-resident; one child process per size, paths alternating inside it"]
    rc = 0
    steps = [("n = %d" % n, ["--step", str(n), str(reps)]) for n in SIZES] + [("hd paths", ["--step-hd", str(reps)])]
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
    with open(os.path.join(out_dir, "keygen_probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
