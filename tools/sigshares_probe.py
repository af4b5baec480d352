"""Signature-share verification (csrc/blsgpu_sigshares.hip) at 10 000 sessions of k = 67 unit signatures over 100 players
(the sharing of tests/golden/threshold.json, every session a different seeded 67-subset, one message), device events:
  * blsgpu_sig_shares_check_dev (scaled) with no bad share, with one bad share in 1 % of the sessions, and with one bad share
    in EVERY session, with the rounds and node tests it reports;
  * in the same run and on the same inputs, alternating, the exact alternative: lambda_i PK_i by blsgpu_g1_msm_dev(k = 1) with
    the coefficients of blsgpu_lagrange_at_zero_dev, H(m) by blsgpu_hash_to_g2_dev, and one two-pair pairing per share,
    blsgpu_pairing_multi_batch_dev(2, groups x k) (the pairs assembled by strided device copies; -G1 and the shares are
    placed once, outside the timed region);
  * blsgpu_threshold_combine_dev on the plain shares sk_i H(m) of the same subsets plus the verification of the 10 000
    combined signatures (hash, two-pair pairings) alone: what a combiner pays today to learn THAT something is wrong.
Every status byte is compared with what was planted.
usage: python3 tools/sigshares_probe.py [out_dir (default profiles)] [repeats (default 5)] [sessions (default 10000)]
Writes <out_dir>/sigshares_probe.txt, stamped with the library's version string and a digest of libblsgpu.so."""
import hashlib
import json
import os
import random
import statistics
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-bls_amd"))
N = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    groups = int(sys.argv[3]) if len(sys.argv) > 3 else 10000
    k = 67

    import torch
    from bls_py import _native, util
    from bls_py import hostmath as H

    eng = _native.Engine(0)
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

    with open(_native._LIB_PATH, "rb") as f:
        lib_digest = hashlib.sha256(f.read()).hexdigest()[:16]
    log("# sigshares_probe: %s, libblsgpu.so sha256 %s, %s, %d sessions x %d shares, %d repeats after 1 warm-up call (median, min, "
        "max; device events, the round synchronisations of the check included)" % (eng.version(), lib_digest, torch.cuda.get_device_name(0), groups, k, reps))

    with open(os.path.join(ROOT, "tests", "golden", "threshold.json")) as f:
        th = json.load(f)["67_of_100"]
    poly = [int(c, 16) for c in th["poly"]]

    def share(x):
        acc = 0
        for c in reversed(poly):
            acc = (acc * x + c) % N
        return acc
    sk = {x: share(x) for x in range(1, 101)}
    mh = util.hash256(bytes.fromhex(th["msg"]))
    hm = eng.hash_to_g2(mh)
    keys, _ = eng.g1_mul_gen(b"".join(sk[x].to_bytes(32, "big") for x in range(1, 101)))
    rnd = random.Random(20000)
    subsets = [rnd.sample(range(1, 101), k) for _ in range(groups)]
    n = groups * k
    x_bytes = b"".join(p.to_bytes(32, "big") for S in subsets for p in S)
    co, status = eng.lagrange_at_zero(x_bytes, k, groups)
    assert status == b"\x01" * groups
    scal = [int.from_bytes(co[32 * i:32 * (i + 1)], "big") * sk[p] % N for i, p in enumerate(p for S in subsets for p in S)]
    unit = bytearray()
    for lo in range(0, n, 100000):                       # unit signatures lambda_i sk_i H(m) on the device, in slices
        m = min(100000, n - lo)
        out, _ = eng.g2_msm(hm * m, scal[lo:lo + m], 1, m)
        unit += out
    wrong, _ = eng.g2_msm(hm * groups, [(scal[g * k + 5] + 1) % N for g in range(groups)], 1, groups)   # share 5 of every session, spoiled
    key_idx = [p - 1 for S in subsets for p in S]
    weights = b"".join((rnd.getrandbits(64) or 1).to_bytes(8, "big") for _ in range(n))

    d_keys, d_idx, d_x = to_dev(keys), to_dev(struct.pack("<%dI" % n, *key_idx)), to_dev(x_bytes)
    d_mh, d_w = to_dev(mh * groups), to_dev(weights)
    d_st = torch.empty(n, dtype=torch.uint8, device=dev)
    d_ss = torch.empty(groups, dtype=torch.uint8, device=dev)
    # the exact alternative's buffers
    d_co = torch.empty(32 * n, dtype=torch.uint8, device=dev)
    d_lst = torch.empty(groups, dtype=torch.uint8, device=dev)
    d_pk = to_dev(b"".join(keys[96 * i:96 * (i + 1)] for i in key_idx))
    d_lpk = torch.empty(96 * n, dtype=torch.uint8, device=dev)
    d_h = torch.empty(192, dtype=torch.uint8, device=dev)
    d_mh1 = to_dev(mh)
    neg_g1 = H.g1_affine_bytes((H.G1_GEN[0], -H.G1_GEN[1] % H.Q))
    d_e = torch.empty(576 * n, dtype=torch.uint8, device=dev)
    one = torch.zeros(576, dtype=torch.uint8, device=dev)
    one[47] = 1

    for name, bad in (("no bad share", []), ("one bad share in 1 % of the sessions", list(range(0, groups, 100))),
                      ("one bad share in every session", list(range(groups)))):
        sig = bytearray(unit)
        for g in bad:
            sig[192 * (g * k + 5):192 * (g * k + 6)] = wrong[192 * g:192 * (g + 1)]
        d_sig = to_dev(sig)
        expect = bytearray(b"\x01" * n)
        for g in bad:
            expect[g * k + 5] = 0
        stats = [None]

        def f_check():
            stats[0] = eng.sig_shares_check_dev(d_sig.data_ptr(), d_keys.data_ptr(), 100, d_idx.data_ptr(), d_x.data_ptr(), d_mh.data_ptr(),
                                                d_w.data_ptr(), True, k, groups, d_st.data_ptr(), d_ss.data_ptr(), st.cuda_stream)
        g1_pairs = torch.empty((n, 2, 96), dtype=torch.uint8, device=dev)
        g2_pairs = torch.empty((n, 2, 192), dtype=torch.uint8, device=dev)
        g1_pairs[:, 0, :] = to_dev(neg_g1)
        g2_pairs[:, 0, :] = d_sig.view(n, 192)

        def f_exact():
            eng.lagrange_at_zero_dev(d_x.data_ptr(), k, groups, d_co.data_ptr(), d_lst.data_ptr(), st.cuda_stream)
            eng._check(eng.lib.blsgpu_g1_msm_dev(eng.h, d_pk.data_ptr(), d_co.data_ptr(), 1, n, d_lpk.data_ptr(), None, st.cuda_stream), "g1_msm_dev")
            eng._check(eng.lib.blsgpu_hash_to_g2_dev(eng.h, d_mh1.data_ptr(), 1, d_h.data_ptr(), st.cuda_stream), "hash_to_g2_dev")
            g1_pairs[:, 1, :] = d_lpk.view(n, 96)                      # (torch copies on the same stream)
            g2_pairs[:, 1, :] = d_h
            eng._check(eng.lib.blsgpu_pairing_multi_batch_dev(eng.h, g1_pairs.data_ptr(), g2_pairs.data_ptr(), None, 2, n, d_e.data_ptr(),
                                                              st.cuda_stream), "pairing_multi_batch_dev")
        timed(f_check)
        timed(f_exact)
        tc, te = [], []
        for _ in range(reps):
            tc.append(timed(f_check))
            te.append(timed(f_exact))
        ok = bytes(d_st.cpu().numpy()) == bytes(expect) and int(d_ss.sum().item()) == groups
        exact = bytes((d_e.view(n, 576) == one).all(dim=1).to(torch.uint8).cpu().numpy())
        log("\n## %s" % name)
        log("blsgpu_sig_shares_check_dev                         %s ms   rounds %d, node tests %d; status as planted: %s"
            % (spread(tc), stats[0][0], stats[0][1], ok))
        log("exact: lambda PK (g1_msm k = 1) + %7d two-pair pairings %s ms   status as planted: %s; check / exact: %.3f"
            % (n, spread(te), exact == bytes(expect), statistics.median(tc) / statistics.median(te)))

    # what a combiner pays today: combine, then verify the combined signature against the master key
    plain = bytearray()
    for lo in range(0, n, 100000):
        m = min(100000, n - lo)
        out, _ = eng.g2_msm(hm * m, [sk[i + 1] for i in key_idx[lo:lo + m]], 1, m)
        plain += out
    d_sig = to_dev(plain)
    d_out = torch.empty(192 * groups, dtype=torch.uint8, device=dev)
    d_inf = torch.empty(groups, dtype=torch.uint8, device=dev)
    master, _ = eng.g1_mul_gen(poly[0].to_bytes(32, "big"))
    g1v = torch.empty((groups, 2, 96), dtype=torch.uint8, device=dev)
    g2v = torch.empty((groups, 2, 192), dtype=torch.uint8, device=dev)
    g1v[:, 0, :] = to_dev(neg_g1)
    g1v[:, 1, :] = to_dev(master)
    d_ev = torch.empty(576 * groups, dtype=torch.uint8, device=dev)
    d_hg = torch.empty(192 * groups, dtype=torch.uint8, device=dev)

    def f_combine():
        eng.threshold_combine_dev(d_sig.data_ptr(), d_x.data_ptr(), k, groups, d_out.data_ptr(), d_inf.data_ptr(), d_lst.data_ptr(), st.cuda_stream)
        eng._check(eng.lib.blsgpu_hash_to_g2_dev(eng.h, d_mh.data_ptr(), groups, d_hg.data_ptr(), st.cuda_stream), "hash_to_g2_dev")
        g2v[:, 0, :] = d_out.view(groups, 192)
        g2v[:, 1, :] = d_hg.view(groups, 192)
        eng._check(eng.lib.blsgpu_pairing_multi_batch_dev(eng.h, g1v.data_ptr(), g2v.data_ptr(), None, 2, groups, d_ev.data_ptr(), st.cuda_stream),
                   "pairing_multi_batch_dev")
    timed(f_combine)
    ts = [timed(f_combine) for _ in range(reps)]
    good = bool((d_ev.view(groups, 576) == one).all().item())
    log("\n## blsgpu_threshold_combine_dev on the plain shares and verify the %d combined signatures: %s ms   all verify: %s"
        % (groups, spread(ts), good))

    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "sigshares_probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    eng.close()


if __name__ == "__main__":
    main()
