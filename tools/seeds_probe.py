"""Keys from seeds on the device (blsgpu_keys_from_seeds_dev, csrc/blsgpu_seeds.hip), timed after warm-up:
  1. 65 536 and 2^20 seeds of 32 and of 64 bytes, PrivateKey.from_seed (plain) and ExtendedPrivateKey.from_seed (hd), every
     output: the whole call by device events, k_seed_keys (timing kind 13) and the multiplication (kind 9) from the
     library's timing records (summed over the slices of a call), and blsgpu_g1_mul_gen_secret_dev alone on the same count --
     the floor the call cannot go below;
  2. the way there was before it: the Python loop of from_seed plus get_public_key_batch(secret=True), host clock, measured
     on a SAMPLE of seeds and SCALED to the count;
  3. seeds -> out_parents -> blsgpu_hd_paths_secret_dev at depth 4 (hardened, hardened, not, not), against masters made on the
     host (the loop of 2 on a sample, scaled, plus the upload of their records) and the same path call.
usage: python3 tools/seeds_probe.py [out_dir (default profiles)] [repeats (default 3)] [sample (default 2048)]
Writes <out_dir>/seeds_probe.txt, stamped with the library's version string and a digest of libblsgpu.so."""
import hashlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-bls_amd"))
import torch  # noqa: E402
from bls_py import _native, backend  # noqa: E402
from bls_py import _native_seeds as S  # noqa: E402
from bls_py.keys import ExtendedPrivateKey, PrivateKey, _pk_affine  # noqa: E402

out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
sample = int(sys.argv[3]) if len(sys.argv) > 3 else 2048
eng = _native.engine(0)
backend.use(backend.HipProvider())
dev = torch.device("cuda", 0)
st = torch.cuda.current_stream(dev)
lines = []
H31 = 1 << 31
COUNTS = (65536, 1 << 20)
DEPTH = 4


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


def kinds(fn):
    """median over the repeats of the summed ms per timing kind of one call"""
    eng.timing_enable(True)
    try:
        eng.timing_read()
        per = []
        for _ in range(reps):
            fn()
            tot = {}
            for k, ms in eng.timing_read():
                tot[k] = tot.get(k, 0.0) + ms
            per.append(tot)
    finally:
        eng.timing_enable(False)
    return {k: statistics.median(p.get(k, 0.0) for p in per) for k in per[0]}


def u8(n):
    return torch.empty(n, dtype=torch.uint8, device=dev)


with open(_native._LIB_PATH, "rb") as f:
    lib_digest = hashlib.sha256(f.read()).hexdigest()[:16]
log("# seeds_probe: %s, libblsgpu.so sha256 %s, %s, medians of %d calls after warm-up (ms)"
    % (eng.version(), lib_digest, torch.cuda.get_device_name(0), reps))

log("\n## 1. blsgpu_keys_from_seeds_dev, every output; kinds 13 / 9 from the timing records; g1_mul_gen_secret_dev alone as the floor")
log("%8s %4s %6s %10s %12s %12s %12s %8s" % ("seeds", "len", "mode", "call", "k_seed_keys", "mul (kind 9)", "mul alone", "hash/mul"))
gen = torch.Generator().manual_seed(0x5eed)
for n in COUNTS:
    sk, chain, aff, ser, par = u8(32 * n), u8(32 * n), u8(96 * n), u8(48 * n), u8(160 * n)
    floor_ms = median(lambda: eng.g1_mul_gen_secret_dev(sk.data_ptr(), n, aff.data_ptr(), ser.data_ptr(), st.cuda_stream))
    for L in (32, 64):
        d_seeds = torch.randint(0, 256, (L * n,), dtype=torch.uint8, generator=gen).to(dev)
        for hd in (False, True):
            def call():
                S.keys_from_seeds_dev(eng, d_seeds.data_ptr(), L, n, hd, sk.data_ptr(), chain.data_ptr() if hd else None, aff.data_ptr(),
                                      ser.data_ptr(), par.data_ptr() if hd else None, st.cuda_stream)
            t = median(call)
            k = kinds(call)
            log("%8d %4d %6s %10.3f %12.3f %12.3f %12.3f %8.4f" % (n, L, "hd" if hd else "plain", t, k[13], k[9], floor_ms, k[13] / k[9]))
    del sk, chain, aff, ser, par

log("\n## 2. before: the Python loop of from_seed + get_public_key_batch(secret=True), host clock, on a SAMPLE of %d seeds, SCALED" % sample)
log("%6s %4s %14s %16s %16s" % ("mode", "len", "sample ms", "scaled to 65536", "scaled to 2^20"))
rnd = __import__("random").Random(0x5eed)
loop_ms = {}
for L in (32, 64):
    seeds = [rnd.randbytes(L) for _ in range(sample)]
    for hd in (False, True):
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            if hd:
                masters = [ExtendedPrivateKey.from_seed(s) for s in seeds]
                keys = [m.private_key for m in masters]
            else:
                keys = [PrivateKey.from_seed(s) for s in seeds]
            PrivateKey.get_public_key_batch(keys, secret=True)
            ts.append((time.perf_counter() - t0) * 1e3)
        t = statistics.median(ts)
        loop_ms[L, hd] = t
        log("%6s %4d %14.3f %16.1f %16.1f" % ("hd" if hd else "plain", L, t, t * 65536 / sample, t * (1 << 20) / sample))

log("\n## 3. seeds (32 bytes) -> out_parents -> blsgpu_hd_paths_secret_dev, depth %d, one path per seed" % DEPTH)
log("host masters: the loop of 2 on the sample SCALED to the count, plus the records built on the sample SCALED, plus their upload and the same path call")
log("%8s %12s %12s %12s %18s %10s" % ("seeds", "seeds ms", "paths ms", "chain ms", "host masters ms", "ratio"))
seeds_s = [rnd.randbytes(32) for _ in range(sample)]
t0 = time.perf_counter()
ms_ = [ExtendedPrivateKey.from_seed(s) for s in seeds_s]
for m, pk in zip(ms_, PrivateKey.get_public_key_batch([m.private_key for m in ms_], secret=True)):
    m.private_key.__dict__["_pk_point"] = pk.value
recs = b"".join(m.chain_code + _pk_affine(m._public_key()) + m.private_key.serialize() for m in ms_)
host_sample_ms = (time.perf_counter() - t0) * 1e3
for n in COUNTS:
    d_seeds = torch.randint(0, 256, (32 * n,), dtype=torch.uint8, generator=gen).to(dev)
    d_par = u8(160 * n)
    d_of = torch.arange(n, dtype=torch.int32, device=dev)
    path = torch.tensor([H31 + 44, H31, 0, 5], dtype=torch.int64).to(torch.int32)
    d_idx = path.repeat(n).contiguous().to(dev)
    outs = [u8(w * n) for w in (32, 32, 96, 48, 4)]
    host_recs = torch.empty(160 * n, dtype=torch.uint8).pin_memory()

    def seeds_call():
        S.keys_from_seeds_dev(eng, d_seeds.data_ptr(), 32, n, True, None, None, None, None, d_par.data_ptr(), st.cuda_stream)

    def paths_call():
        eng.hd_paths_secret_dev(d_par.data_ptr(), n, d_of.data_ptr(), d_idx.data_ptr(), DEPTH, n, *[o.data_ptr() for o in outs], st.cuda_stream)

    def chain():
        seeds_call()
        paths_call()

    def upload_and_paths():
        d_par.copy_(host_recs, non_blocking=True)
        paths_call()

    t_seeds, t_paths, t_chain, t_up = median(seeds_call), median(paths_call), median(chain), median(upload_and_paths)
    host_total = host_sample_ms * n / sample + t_up
    log("%8d %12.3f %12.3f %12.3f %18.1f %10.1f" % (n, t_seeds, t_paths, t_chain, host_total, host_total / t_chain))
    del d_seeds, d_par, d_of, d_idx, outs, host_recs

os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "seeds_probe.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
