"""Fixed-base G1 kernel and HD derivation, timed with device events after warm-up (csrc/blsgpu_g1fix.hip):
  * blsgpu_g1_mul_gen_dev against blsgpu_g1_msm_dev(k = 1, groups = n) -- the variable-base path every s G1 took
    before -- on the same scalars, alternating in one process, n = 1, 4096, 65 536, 2^20 (outputs compared);
  * blsgpu_hd_children_dev, public and private mode, 65 536 and 2^20 children;
  * ExtendedPublicKey.public_child_batch(range(65536)) end to end in Python (host clock).
usage: python3 tools/hd_probe.py [out_dir (default profiles)] [repeats (default 5)]
Writes <out_dir>/hd_probe.txt, stamped with the library's version string and a digest of libblsgpu.so."""
import hashlib
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-bls_amd"))
import torch  # noqa: E402
from bls_py import _native  # noqa: E402
from bls_py import hostmath as H  # noqa: E402

out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
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


with open(_native._LIB_PATH, "rb") as f:
    lib_digest = hashlib.sha256(f.read()).hexdigest()[:16]
log("# hd_probe: %s, libblsgpu.so sha256 %s, %s, %d repeats (median ms, device events, after warm-up)"
    % (eng.version(), lib_digest, torch.cuda.get_device_name(0), reps))

rnd = random.Random(1)
G = H.g1_affine_bytes(H.G1_GEN)
log("\n## s G1: fixed-base table (g1_mul_gen) vs variable-base (g1_msm k=1, groups=n), alternating")
log("%9s %12s %12s %8s %s" % ("n", "mul_gen ms", "g1_msm ms", "ratio", "outputs equal"))
for n in (1, 4096, 65536, 1 << 20):
    sc = bytearray(rnd.getrandbits(8) for _ in range(32 * n)) if n <= 65536 else bytearray(os.urandom(32 * n))
    d_sc = torch.frombuffer(sc, dtype=torch.uint8).to(dev)
    d_pts = torch.frombuffer(bytearray(G * n), dtype=torch.uint8).to(dev)
    d_a = torch.zeros(96 * n, dtype=torch.uint8, device=dev)
    d_b = torch.zeros(96 * n, dtype=torch.uint8, device=dev)
    d_inf = torch.zeros(n, dtype=torch.uint8, device=dev)
    f_fix = lambda: eng.g1_mul_gen_dev(d_sc.data_ptr(), n, d_a.data_ptr(), None, st.cuda_stream)
    f_msm = lambda: eng._check(eng.lib.blsgpu_g1_msm_dev(eng.h, d_pts.data_ptr(), d_sc.data_ptr(), 1, n, d_b.data_ptr(),
                                                         d_inf.data_ptr(), st.cuda_stream), "g1_msm_dev")
    for _ in range(2):
        timed(f_fix)
        timed(f_msm)
    tf, tm = [], []
    for _ in range(reps):
        tf.append(timed(f_fix))
        tm.append(timed(f_msm))
    same = bool(torch.equal(d_a, d_b))
    mf, mm = statistics.median(tf), statistics.median(tm)
    log("%9d %12.3f %12.3f %8.2f %s" % (n, mf, mm, mm / mf, same))
    del d_sc, d_pts, d_a, d_b, d_inf
    torch.cuda.empty_cache()

log("\n## hd_children_dev (HMACs + keys on the device; public mode includes its index check and one stream sync)")
log("%9s %8s %12s %14s" % ("n", "mode", "ms", "children/s"))
chain = bytes(range(32))
pk = G
sk = (12345).to_bytes(32, "big")
for n in (65536, 1 << 20):
    d_idx = torch.arange(n, dtype=torch.int32, device=dev)
    d_chain = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
    d_sk = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
    d_aff = torch.zeros(96 * n, dtype=torch.uint8, device=dev)
    d_ser = torch.zeros(48 * n, dtype=torch.uint8, device=dev)
    for mode, psk in (("public", None), ("private", sk)):
        f = lambda: eng.hd_children_dev(chain, pk, psk, d_idx.data_ptr(), n, d_chain.data_ptr(), d_sk.data_ptr() if psk else None,
                                        d_aff.data_ptr(), d_ser.data_ptr(), st.cuda_stream)
        for _ in range(2):
            timed(f)
        t = statistics.median(timed(f) for _ in range(reps))
        log("%9d %8s %12.3f %14.3e" % (n, mode, t, n / (t / 1e3)))
    del d_idx, d_chain, d_sk, d_aff, d_ser
    torch.cuda.empty_cache()

log("\n## ExtendedPublicKey.public_child_batch(range(65536)), Python end to end (host clock)")
from bls_py.keys import ExtendedPrivateKey  # noqa: E402
xpub = ExtendedPrivateKey.from_seed(b"hd_probe").get_extended_public_key()
xpub.public_child_batch(range(64))
ts = []
for _ in range(3):
    t0 = time.perf_counter()
    kids = xpub.public_child_batch(range(65536))
    ts.append((time.perf_counter() - t0) * 1e3)
one = xpub.public_child(65535)
log("65536 children: %.1f ms median of 3 (%.2f us per child); child 65535 equals public_child(65535): %s"
    % (statistics.median(ts), statistics.median(ts) * 1e3 / 65536, kids[-1] == one))
t0 = time.perf_counter()
for i in range(20):
    xpub.public_child(i)
log("public_child one at a time: %.2f ms per child" % ((time.perf_counter() - t0) * 1e3 / 20))

os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "hd_probe.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
eng.close()
