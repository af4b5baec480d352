"""The receiving side of key generation for secrets against the default paths, device-resident with device events after
warm-up, the two forms alternating in one process per step on the same inputs:
  check T N dealers [player]  (s) blsgpu_g1_poly_check_secret_dev (k_poly_eval_secret, csrc/blsgpu_g1poly.hip) against
                              (d) blsgpu_g1_poly_check_dev on the dealers x N fragment matrix of a dealing made on the device
                              (blsgpu_threshold_deal_secret_dev) -- or, with `player`, on the one column a single player
                              receives: `dealers` fragments, one per polynomial.  Both forms share k_poly_prep and
                              k_poly_subgroup, which dominate the small calls.
  sum k groups                (s) blsgpu_fr_sum_secret_dev with both key outputs (k_fr_sum_secret, then k_fix_mul_secret on the
                              sums) against (d) the host loop of BLS.aggregate_priv_keys + get_public_key's arithmetic --
                              Python integers and one blsgpu_g1_mul_gen round trip per key -- timed by the wall clock on
                              HOST_GROUPS groups.
Each is reported as min and median of the repeats; the outputs of the two forms are compared in the same run.
No ratio is required: the secret left-hand side does 65 additions where the default does 32.

usage: python3 tools/rx_probe.py [out_dir (default profiles)] [repeats (default 20)]
The driver makes no GPU call itself: every step is a child process of its own under `timeout`, and the first child that
fails ends the run.  Writes <out_dir>/rx_probe.txt, stamped with the library's version string and a digest of libblsgpu.so."""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-bls_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from deal_probe import N_ORDER, _report, _scalars, _setup  # noqa: E402
from keygen_probe import _alternate  # noqa: E402

CHECKS = ((67, 100, 100, 0), (67, 100, 100, 7), (667, 1000, 1000, 0))     # T, N, dealers, player (0: the whole matrix)
SUM = (100, 10000)
HOST_GROUPS = 20
BIG_REPEATS = 5                                                          # the 1000 x 1000 matrix: seconds per call
STEP_SECONDS = 420


def step_check(T, N, dealers, player, reps):
    what = "the %d x %d matrix" % (dealers, N) if not player else "player %d's %d fragments" % (player, dealers)
    torch, eng, dev, st = _setup("verify_secret_fragment_batch, T = %d, %s" % (T, what), reps)
    d_co = _scalars(torch, torch.Generator().manual_seed(T * N + 1), dealers * T).to(dev)
    d_xs = torch.tensor(list(b"".join(x.to_bytes(32, "big") for x in range(1, N + 1))), dtype=torch.uint8, device=dev)
    d_commit = torch.zeros(96 * dealers * T, dtype=torch.uint8, device=dev)
    d_frag = torch.zeros(32 * dealers * N, dtype=torch.uint8, device=dev)
    s = st.cuda_stream
    eng.threshold_deal_secret_dev(d_co.data_ptr(), dealers, T, d_xs.data_ptr(), N, d_commit.data_ptr(), d_frag.data_ptr(), s)
    if player:
        n = dealers
        d_poly = torch.arange(dealers, dtype=torch.int32, device=dev)
        d_x = d_xs.reshape(N, 32)[player - 1].repeat(dealers).contiguous()
        d_s = d_frag.reshape(dealers, N, 32)[:, player - 1, :].reshape(-1).contiguous()
    else:
        n = dealers * N
        d_poly = torch.arange(dealers, dtype=torch.int32, device=dev).repeat_interleave(N).contiguous()
        d_x = d_xs.repeat(dealers).contiguous()
        d_s = d_frag.clone()
    d_s[32 * (n // 2) + 31] ^= 1                                          # one wrong fragment
    d_ss, d_sd = (torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(2))
    d_as, d_ad = (torch.zeros(96 * n, dtype=torch.uint8, device=dev) for _ in range(2))
    a = (d_commit.data_ptr(), dealers, T, d_poly.data_ptr(), d_x.data_ptr(), d_s.data_ptr(), n)
    forms = (("s", lambda: eng.g1_poly_check_secret_dev(*a, d_ss.data_ptr(), d_as.data_ptr(), s)),
             ("d", lambda: eng.g1_poly_check_dev(*a, d_sd.data_ptr(), d_ad.data_ptr(), s)))
    t = _alternate(st, forms, reps)
    _report(t, {"s": "(s) g1_poly_check_secret_dev", "d": "(d) g1_poly_check_dev"}, "fragments", n)
    print("status equal: %s, Horner values equal: %s, fragments refused: %d of %d (1 tampered)"
          % (bool(torch.equal(d_ss, d_sd)), bool(torch.equal(d_as, d_ad)), int((d_ss != 1).sum()), n), flush=True)
    eng.close()


def step_sum(k, groups, reps):
    torch, eng, dev, st = _setup("aggregate_priv_keys_batch with public keys, %d groups of %d" % (groups, k), reps)
    y = _scalars(torch, torch.Generator().manual_seed(k + groups), k * groups)
    d_y = y.to(dev)
    d_out, d_aff, d_ser = (torch.zeros(w * groups, dtype=torch.uint8, device=dev) for w in (32, 96, 48))
    s = st.cuda_stream
    forms = (("s", lambda: eng.fr_sum_secret_dev(d_y.data_ptr(), k, groups, d_out.data_ptr(), d_aff.data_ptr(), d_ser.data_ptr(), s)),)
    t = _alternate(st, forms, reps)
    print("%-44s %10s %10s %14s" % ("path", "min", "median", "groups/s"))
    med = statistics.median(t["s"])
    print("%-44s %10.3f %10.3f %14.3e" % ("(s) fr_sum_secret_dev, sums and keys", min(t["s"]), med, groups / med * 1e3))
    m = min(groups, HOST_GROUPS)
    raw = bytes(y[:32 * m * k].tolist())
    ints = [int.from_bytes(raw[32 * i:32 * (i + 1)], "big") for i in range(m * k)]
    t0 = time.perf_counter()
    host, host_aff = [], []
    for g in range(m):
        total = sum(ints[g * k:(g + 1) * k]) % N_ORDER
        host.append(total)
        host_aff.append(eng.g1_mul_gen(total.to_bytes(32, "big"), ser=False)[0])      # one round trip per key, as get_public_key makes
    wall = time.perf_counter() - t0
    print("(d) host loop on %d of the %d groups: %.3f s wall clock (%.3f ms per group; the other %d NOT MEASURED)"
          % (m, groups, wall, wall / m * 1e3, groups - m))
    print("sums of those equal the device's: %s, keys: %s"
          % (bytes(d_out[:32 * m].cpu().tolist()) == b"".join(v.to_bytes(32, "big") for v in host),
             bytes(d_aff[:96 * m].cpu().tolist()) == b"".join(host_aff)), flush=True)
    eng.close()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--step-check":
        step_check(*(int(a) for a in sys.argv[2:7]))
        return 0
    if len(sys.argv) > 1 and sys.argv[1] == "--step-sum":
        step_sum(*(int(a) for a in sys.argv[2:5]))
        return 0
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
    reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 20
    lines = ["# rx_probe: the share check and the share sums for secrets against the default paths, device-resident; one child process per step"]
    rc = 0
    steps = [("check %d %d %d %d" % c, ["--step-check"] + [str(v) for v in c] + [str(reps if c[1] * c[2] < 10**6 else min(reps, BIG_REPEATS))])
             for c in CHECKS]
    steps.append(("sum", ["--step-sum", str(SUM[0]), str(SUM[1]), str(reps)]))
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
    with open(os.path.join(out_dir, "rx_probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
