"""The threshold calls for secrets against the default paths, device-resident with device events after warm-up
(csrc/blsgpu_frsecret.hip), the two forms alternating in one process per step on the same inputs:
  deal T N count   (s) blsgpu_threshold_deal_secret_dev: count x T commitments on k_fix_mul_secret and count x N fragments on
                       k_fr_poly_eval_secret;
                   (d) the device half of the default PrivateKey.new_threshold_batch: blsgpu_g1_mul_gen_dev for the
                       commitments.  Its fragments are a Python big-integer Horner loop on the host, which no device event
                       sees: it is timed by the wall clock on at most HOST_POLYS polynomials and reported beside (d).
  interpolate      (s) blsgpu_fr_interpolate_at_zero_secret_dev against (d) blsgpu_fr_interpolate_at_zero_dev, 10 000 x 67.
  sign k           (s) blsgpu_sign_threshold_dev, one session of k signers, against (d) the device calls of the default
                       PrivateKey.sign_threshold_batch: blsgpu_lagrange_at_zero_dev, blsgpu_hash_to_g2_dev and
                       blsgpu_g2_msm_dev(k = 1, groups = k) (its lambda sk mod n is a host multiplication, not timed).
Each is reported as min and median of the repeats; the outputs of the two forms are compared where both are on the device.
No ratio is required: the secret forms do strictly more work on the G1 / G2 side.

usage: python3 tools/deal_probe.py [out_dir (default profiles)] [repeats (default 20)]
The driver makes no GPU call itself: every step is a child process of its own under `timeout`, and the first child that
fails ends the run.  Writes <out_dir>/deal_probe.txt, stamped with the library's version string and a digest of
libblsgpu.so."""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-bls_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from keygen_probe import _alternate, _head  # noqa: E402

DEALS = ((67, 100, 100), (667, 1000, 1000))
INTERP = (10000, 67)
SIGN_K = 67
HOST_POLYS = 10
STEP_SECONDS = 240
N_ORDER = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def _report(t, names, unit, count):
    print("%-44s %10s %10s %14s" % ("path", "min", "median", unit + "/s"))
    for k in names:
        med = statistics.median(t[k])
        print("%-44s %10.3f %10.3f %14.3e" % (names[k], min(t[k]), med, count / med * 1e3))
    print("(s) / (d) = %.3f on medians (recorded)" % (statistics.median(t["s"]) / statistics.median(t["d"])), flush=True)


def _setup(what, reps):
    import torch
    from bls_py import _native
    eng = _native.Engine(0)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    _head(what, eng, reps)
    return torch, eng, dev, st


def _scalars(torch, gen, n):
    sc = torch.randint(0, 256, (n, 32), dtype=torch.uint8, generator=gen)
    sc[:, 0] &= 0x3F                                     # below 2^254 < n
    return sc.reshape(-1)


def step_deal(T, N, count, reps):
    torch, eng, dev, st = _setup("new_threshold_batch(%d, %d, %d)" % (T, N, count), reps)
    gen = torch.Generator().manual_seed(T * N)
    co = _scalars(torch, gen, count * T)
    d_co = co.to(dev)
    d_x = torch.tensor(list(b"".join(x.to_bytes(32, "big") for x in range(1, N + 1))), dtype=torch.uint8, device=dev)
    d_cs, d_cd = (torch.zeros(96 * count * T, dtype=torch.uint8, device=dev) for _ in range(2))
    d_fr = torch.zeros(32 * count * N, dtype=torch.uint8, device=dev)
    s = st.cuda_stream
    forms = (("s", lambda: eng.threshold_deal_secret_dev(d_co.data_ptr(), count, T, d_x.data_ptr(), N, d_cs.data_ptr(), d_fr.data_ptr(), s)),
             ("d", lambda: eng.g1_mul_gen_dev(d_co.data_ptr(), count * T, d_cd.data_ptr(), None, s)))
    t = _alternate(st, forms, reps)
    _report(t, {"s": "(s) threshold_deal_secret_dev", "d": "(d) g1_mul_gen_dev (commitments only)"}, "dealings", count)
    print("commitments equal: %s" % bool(torch.equal(d_cs, d_cd)))
    polys = min(count, HOST_POLYS)
    raw = bytes(co[:32 * polys * T].tolist())
    ints = [int.from_bytes(raw[32 * i:32 * (i + 1)], "big") for i in range(polys * T)]
    t0 = time.perf_counter()
    host = []
    for p in range(polys):
        poly = ints[p * T:(p + 1) * T]
        for x in range(1, N + 1):
            acc = 0
            for c in reversed(poly):
                acc = (acc * x + c) % N_ORDER
            host.append(acc)
    wall = time.perf_counter() - t0
    got = bytes(d_fr[:32 * polys * N].cpu().tolist())
    print("(d) host Horner of %d of the %d polynomials: %.3f s wall clock (%.1f ms per polynomial; the other %d NOT MEASURED)"
          % (polys, count, wall, wall / polys * 1e3, count - polys))
    print("fragments of those equal the device's: %s" % (got == b"".join(v.to_bytes(32, "big") for v in host)), flush=True)
    eng.close()


def step_interpolate(reps):
    groups, k = INTERP
    torch, eng, dev, st = _setup("interpolate_at_zero, %d x %d" % (groups, k), reps)
    import random
    rnd = random.Random(3)
    x = b"".join(v.to_bytes(32, "big") for _ in range(groups) for v in rnd.sample(range(1, 101), k))
    d_x = torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev)
    d_y = _scalars(torch, torch.Generator().manual_seed(5), groups * k).to(dev)
    d_s, d_d = (torch.zeros(32 * groups, dtype=torch.uint8, device=dev) for _ in range(2))
    d_st = torch.zeros(groups, dtype=torch.uint8, device=dev)
    s = st.cuda_stream
    forms = (("s", lambda: eng.fr_interpolate_at_zero_secret_dev(d_x.data_ptr(), d_y.data_ptr(), k, groups, d_s.data_ptr(), d_st.data_ptr(), s)),
             ("d", lambda: eng.fr_interpolate_at_zero_dev(d_x.data_ptr(), d_y.data_ptr(), k, groups, d_d.data_ptr(), d_st.data_ptr(), s)))
    t = _alternate(st, forms, reps)
    _report(t, {"s": "(s) fr_interpolate_at_zero_secret_dev", "d": "(d) fr_interpolate_at_zero_dev"}, "groups", groups)
    print("outputs equal: %s, every status 1: %s" % (bool(torch.equal(d_s, d_d)), bool((d_st == 1).all())), flush=True)
    eng.close()


def step_sign(k, reps):
    torch, eng, dev, st = _setup("sign_threshold_batch, one session of k = %d" % k, reps)
    players = list(range(1, k + 1))
    x = b"".join(v.to_bytes(32, "big") for v in players)
    d_x = torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev)
    sk = _scalars(torch, torch.Generator().manual_seed(k), k)
    d_sk = sk.to(dev)
    d_h = torch.arange(32, dtype=torch.uint8).to(dev)
    d_s, d_d = (torch.zeros(192 * k, dtype=torch.uint8, device=dev) for _ in range(2))
    d_inf, d_st = torch.zeros(k, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.uint8, device=dev)
    d_co, d_hm = torch.zeros(32 * k, dtype=torch.uint8, device=dev), torch.zeros(192, dtype=torch.uint8, device=dev)
    s = st.cuda_stream
    # the default path's scalars, once (host): lambda_i sk_i mod n
    eng.lagrange_at_zero_dev(d_x.data_ptr(), k, 1, d_co.data_ptr(), d_st.data_ptr(), s)
    co, raw = bytes(d_co.cpu().tolist()), bytes(sk.tolist())
    scal = b"".join((int.from_bytes(co[32 * i:32 * i + 32], "big") * int.from_bytes(raw[32 * i:32 * i + 32], "big") % N_ORDER).to_bytes(32, "big")
                    for i in range(k))
    d_scal = torch.frombuffer(bytearray(scal), dtype=torch.uint8).to(dev)

    def default():
        eng.lagrange_at_zero_dev(d_x.data_ptr(), k, 1, d_co.data_ptr(), d_st.data_ptr(), s)
        eng._check(eng.lib.blsgpu_hash_to_g2_dev(eng.h, d_h.data_ptr(), 1, d_hm.data_ptr(), s), "hash_to_g2_dev")
        d_pts = d_hm.repeat(k)
        eng._check(eng.lib.blsgpu_g2_msm_dev(eng.h, d_pts.data_ptr(), d_scal.data_ptr(), 1, k, d_d.data_ptr(), d_inf.data_ptr(), s), "g2_msm_dev")
    forms = (("s", lambda: eng.sign_threshold_dev(d_sk.data_ptr(), d_x.data_ptr(), k, 1, d_h.data_ptr(), 1, d_s.data_ptr(), None,
                                                  d_inf.data_ptr(), d_st.data_ptr(), s)),
             ("d", default))
    t = _alternate(st, forms, reps)
    _report(t, {"s": "(s) sign_threshold_dev", "d": "(d) lagrange + hash_to_g2 + g2_msm_dev(k=1)"}, "signatures", k)
    print("outputs equal: %s" % bool(torch.equal(d_s, d_d)), flush=True)
    eng.close()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step-deal":
        step_deal(*(int(a) for a in sys.argv[2:6]))
        return 0
    if len(sys.argv) > 1 and sys.argv[1] == "--step-interpolate":
        step_interpolate(int(sys.argv[2]))
        return 0
    if len(sys.argv) > 1 and sys.argv[1] == "--step-sign":
        step_sign(int(sys.argv[2]), int(sys.argv[3]))
        return 0
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
    reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 20
    lines = ["# deal_probe: the threshold calls for secrets against the default paths, device-resident; one child process per step"]
    rc = 0
    steps = [("deal %d %d %d" % d, ["--step-deal"] + [str(v) for v in d] + [str(reps)]) for d in DEALS]
    steps += [("interpolate", ["--step-interpolate", str(reps)]), ("sign", ["--step-sign", str(SIGN_K), str(reps)])]
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
    with open(os.path.join(out_dir, "deal_probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
