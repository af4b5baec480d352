"""Device signing, timed device-resident with device events after warm-up (csrc/blsgpu_g2smul.hip), at 4096 and 65 536
signatures, the three forms alternating in one process per size:
  (a) the composition sign_batch uses: blsgpu_hash_to_g2_dev + blsgpu_g2_msm_dev(k = 1, groups = n);
  (b) blsgpu_sign_dev with distinct messages;
  (c) blsgpu_sign_dev with one message (one hash, one shared table).
Each is reported as min and median of the repeats; for (b) and (c) also the share of k_g2_smul with its table kernel
alone (blsgpu_timing_read, kind 8; the rest of the call is the hash to G2).  The outputs of (a) and (b) are compared.
Goal for (b): (b) <= (a) within the larger of (a)'s own min-to-median spread and 5 %; goal for (c): faster than (b).

usage: python3 tools/sign_probe.py [out_dir (default profiles)] [repeats (default 20)]
The driver makes no GPU call itself: every size is a child process of its own under `timeout`, and the first child that
fails ends the run.  Writes <out_dir>/sign_probe.txt, stamped with the library's version string and a digest of
libblsgpu.so."""
import hashlib
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-bls_amd"))
SIZES = (4096, 65536)
STEP_SECONDS = 240


def step(n, reps):
    import torch
    from bls_py import _native
    eng = _native.Engine(0)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    with open(_native._LIB_PATH, "rb") as f:
        digest = hashlib.sha256(f.read()).hexdigest()[:16]
    print("## n = %d: %s, libblsgpu.so sha256 %s, %s, %d repeats after 3 warm-up rounds (ms, device events)"
          % (n, eng.version(), digest, torch.cuda.get_device_name(0), reps), flush=True)
    gen = torch.Generator().manual_seed(n)
    d_h = torch.randint(0, 256, (32 * n,), dtype=torch.uint8, generator=gen).to(dev)
    sk = torch.randint(0, 256, (n, 32), dtype=torch.uint8, generator=gen)
    sk[:, 0] &= 0x3F                                     # below 2^254 < n: what a private key is
    d_sk = sk.reshape(-1).to(dev)
    d_pts = torch.zeros(192 * n, dtype=torch.uint8, device=dev)
    d_a = torch.zeros(192 * n, dtype=torch.uint8, device=dev)
    d_b = torch.zeros(192 * n, dtype=torch.uint8, device=dev)
    d_c = torch.zeros(192 * n, dtype=torch.uint8, device=dev)
    d_inf = torch.zeros(n, dtype=torch.uint8, device=dev)
    s = st.cuda_stream

    def f_a():
        eng._check(eng.lib.blsgpu_hash_to_g2_dev(eng.h, d_h.data_ptr(), n, d_pts.data_ptr(), s), "hash_to_g2_dev")
        eng._check(eng.lib.blsgpu_g2_msm_dev(eng.h, d_pts.data_ptr(), d_sk.data_ptr(), 1, n, d_a.data_ptr(), d_inf.data_ptr(), s), "g2_msm_dev")

    def f_b():
        eng.sign_dev(d_sk.data_ptr(), d_h.data_ptr(), n, n, d_b.data_ptr(), None, s)

    def f_c():
        eng.sign_dev(d_sk.data_ptr(), d_h.data_ptr(), 1, n, d_c.data_ptr(), None, s)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        return a.elapsed_time(b)

    forms = (("a", f_a), ("b", f_b), ("c", f_c))
    for _ in range(3):
        for _, fn in forms:
            timed(fn)
    t = {k: [] for k, _ in forms}
    kern = {"b": [], "c": []}
    eng.timing_enable(True)
    eng.timing_read()
    for _ in range(reps):
        for k, fn in forms:
            t[k].append(timed(fn))
            rec = eng.timing_read()
            if k in kern:
                kern[k].append(sum(ms for kind, ms in rec if kind == 8))
    eng.timing_enable(False)
    print("%-46s %10s %10s %16s" % ("form", "min", "median", "k_g2_smul median"))
    names = {"a": "(a) hash_to_g2_dev + g2_msm_dev(k=1)", "b": "(b) sign_dev, n messages", "c": "(c) sign_dev, one message"}
    for k, _ in forms:
        print("%-46s %10.3f %10.3f %16s" % (names[k], min(t[k]), statistics.median(t[k]),
                                            "%.3f" % statistics.median(kern[k]) if k in kern else "-"))
    a_min, a_med = min(t["a"]), statistics.median(t["a"])
    b_med, c_med = statistics.median(t["b"]), statistics.median(t["c"])
    margin = max((a_med - a_min) / a_min, 0.05)
    print("outputs of (a) and (b) equal: %s" % bool(torch.equal(d_a, d_b)))
    print("(b) / (a) = %.3f on medians; margin max(spread of (a) %.1f %%, 5 %%) = %.1f %%: goal (b) <= (a) %s"
          % (b_med / a_med, 100 * (a_med - a_min) / a_min, 100 * margin, "met" if b_med <= a_med * (1 + margin) else "MISSED"))
    print("(c) / (b) = %.3f on medians: (c) faster than (b): %s" % (c_med / b_med, c_med < b_med))
    print("signatures per second, medians: (a) %.3e  (b) %.3e  (c) %.3e" % (n / a_med * 1e3, n / b_med * 1e3, n / c_med * 1e3), flush=True)
    eng.close()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step":
        step(int(sys.argv[2]), int(sys.argv[3]))
        return 0
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
    reps = max(20, int(sys.argv[2])) if len(sys.argv) > 2 else 20
    lines = ["# sign_probe: device signing, device-resident; one child process per size, forms alternating inside it"]
    rc = 0
    for n in SIZES:
        p = subprocess.run(["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--step", str(n), str(reps)],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        print(p.stdout, end="", flush=True)
        lines += ["", *p.stdout.rstrip("\n").split("\n")]
        if p.returncode != 0:
            rc = p.returncode
            lines.append("step n = %d ended with status %d: stopped here" % (n, rc))
            print(lines[-1], flush=True)
            break
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "sign_probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
