"""Hash to G1 on the device (blsgpu_hash_to_g1_dev / blsgpu_map_to_g1_dev, csrc/blsgpu_h2g1.hip), timed after warm-up:
  1. hash_to_g1 and map_to_g1 at 4096, 65 536 and 2^20 messages, affine and compressed outputs and the flags, and
     blsgpu_hash_to_g2_dev on the same counts in the same run for scale: whole calls by device events;
  2. the host function (hostmath.hash_to_g1_prehashed, what ec.hash_to_point_prehashed_Fq runs), host clock, on a SAMPLE of
     20 messages and SCALED to the counts;
  3. a seeded comparison of 2000 random message hashes with hostmath, reported as mismatches out of 2000.
usage: python3 tools/h2g1_probe.py [out_dir (default profiles)] [repeats (default 3)] [compared (default 2000)]
Writes <out_dir>/h2g1_probe.txt, stamped with the library's version string and a digest of libblsgpu.so."""
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
from bls_py import _native_h2g1 as G  # noqa: E402
from bls_py import hostmath as H  # noqa: E402
from bls_py.util import hash512  # noqa: E402

out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
compared = int(sys.argv[3]) if len(sys.argv) > 3 else 2000
SAMPLE = 20
COUNTS = (4096, 65536, 1 << 20)
eng = _native.engine(0)
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


def median(fn, warm=1):
    for _ in range(warm):
        timed(fn)
    return statistics.median(timed(fn) for _ in range(reps))


def u8(n):
    return torch.empty(n, dtype=torch.uint8, device=dev)


with open(_native._LIB_PATH, "rb") as f:
    lib_digest = hashlib.sha256(f.read()).hexdigest()[:16]
log("# h2g1_probe: %s, libblsgpu.so sha256 %s, %s, medians of %d calls after warm-up (ms)"
    % (eng.version(), lib_digest, torch.cuda.get_device_name(0), reps))

log("\n## 1. whole _dev calls by device events; hash_to_g2_dev on the same counts for scale")
log("%8s %14s %14s %14s %16s %16s" % ("messages", "hash_to_g1 ms", "map_to_g1 ms", "hash_to_g2 ms", "hash_to_g1 msg/s", "hash_to_g2 msg/s"))
gen = torch.Generator().manual_seed(0x68326731)
for n in COUNTS:
    d_h = torch.randint(0, 256, (32 * n,), dtype=torch.uint8, generator=gen).to(dev)
    d_t = torch.randint(0, 256, (96 * n,), dtype=torch.uint8, generator=gen).to(dev)     # any value below 2^384 is a field element
    aff, ser, inf, g2 = u8(96 * n), u8(48 * n), u8(n), u8(192 * n)
    t_hash = median(lambda: G.hash_to_g1_dev(eng, d_h.data_ptr(), n, aff.data_ptr(), ser.data_ptr(), inf.data_ptr(), st.cuda_stream))
    t_map = median(lambda: G.map_to_g1_dev(eng, d_t.data_ptr(), n, aff.data_ptr(), ser.data_ptr(), inf.data_ptr(), st.cuda_stream))
    t_g2 = median(lambda: eng.lib.blsgpu_hash_to_g2_dev(eng.h, d_h.data_ptr(), n, g2.data_ptr(), st.cuda_stream))
    log("%8d %14.3f %14.3f %14.3f %16.0f %16.0f" % (n, t_hash, t_map, t_g2, n / t_hash * 1e3, n / t_g2 * 1e3))
    del d_h, d_t, aff, ser, inf, g2

log("\n## 2. before: hostmath.hash_to_g1_prehashed, host clock, on a SAMPLE of %d messages, SCALED" % SAMPLE)
rnd = random.Random(0x68326731)
msgs = [rnd.randbytes(32) for _ in range(SAMPLE)]
ts = []
for _ in range(reps):
    t0 = time.perf_counter()
    for m in msgs:
        H.hash_to_g1_prehashed(m, hash512)
    ts.append((time.perf_counter() - t0) * 1e3)
t = statistics.median(ts)
log("%12s %12s %s" % ("sample ms", "per message", "  ".join("scaled to %d" % n for n in COUNTS)))
log("%12.3f %12.3f %s" % (t, t / SAMPLE, "  ".join("%14.1f" % (t * n / SAMPLE) for n in COUNTS)))

log("\n## 3. %d seeded random message hashes against hostmath.hash_to_g1_prehashed (affine bytes, compressed bytes, flag)" % compared)
hashes = [rnd.randbytes(32) for _ in range(compared)]
aff, ser, inf = G.hash_to_g1(eng, b"".join(hashes), aff=True, ser=True)
bad = 0
for i, m in enumerate(hashes):
    A = H.hash_to_g1_prehashed(m, hash512)
    if (aff[96 * i:96 * (i + 1)], ser[48 * i:48 * (i + 1)], inf[i]) != (H.g1_affine_bytes(A), H.g1_compress(A), A is None):
        bad += 1
log("mismatches: %d out of %d" % (bad, compared))

os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "h2g1_probe.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
