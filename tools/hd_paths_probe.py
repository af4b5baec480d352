"""HD path derivation with a parent per lane (blsgpu_hd_paths_dev, csrc/blsgpu_g1fix.hip), timed with device events after
warm-up against the only way there was before it -- one blsgpu_hd_children_dev call per parent and level -- alternating
in one process:
  1. the 256 x 256 public grid m/a/i: one hd_paths_dev call over 65 536 (parent, index) lanes against 256 hd_children_dev
     calls (outputs compared);
  2. 65 536 and 2^20 private paths of depth 4 (hardened, hardened, not, not) in one call, against four rounds of
     per-parent calls timed on a SAMPLE of prefixes and SCALED to the number of distinct prefixes;
  3. depth 1 from one parent against hd_children_dev on the same indices: what per-lane midstates cost where they are
     not needed;
  4. ExtendedPublicKey.public_paths_from for the grid end to end in Python (host clock).
usage: python3 tools/hd_paths_probe.py [out_dir (default profiles)] [repeats (default 5)]
Writes <out_dir>/hd_paths_probe.txt, stamped with the library's version string and a digest of libblsgpu.so."""
import hashlib
import os
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
H31 = 1 << 31


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


def alternate(f, g):
    """medians of f and g, alternating, after two warm-up rounds"""
    for _ in range(2):
        timed(f)
        timed(g)
    tf, tg = [], []
    for _ in range(reps):
        tf.append(timed(f))
        tg.append(timed(g))
    return statistics.median(tf), statistics.median(tg)


def u8(n):
    return torch.zeros(n, dtype=torch.uint8, device=dev)


def i32(values):
    return torch.tensor(values, dtype=torch.int64, device=dev).to(torch.int32)


with open(_native._LIB_PATH, "rb") as f:
    lib_digest = hashlib.sha256(f.read()).hexdigest()[:16]
log("# hd_paths_probe: %s, libblsgpu.so sha256 %s, %s, %d repeats (median ms, device events, after warm-up)"
    % (eng.version(), lib_digest, torch.cuda.get_device_name(0), reps))

G = H.g1_affine_bytes(H.G1_GEN)
root_chain = bytes(range(32))

log("\n## 1. public grid 256 x 256: one hd_paths_dev call vs 256 hd_children_dev calls (one per parent), alternating")
A = I = 256
acc_chain, _, acc_aff, _ = eng.hd_children(root_chain, G, None, list(range(A)))
records = b"".join(acc_chain[32 * a:32 * a + 32] + acc_aff[96 * a:96 * a + 96] + bytes(32) for a in range(A))
d_par = torch.frombuffer(bytearray(records), dtype=torch.uint8).to(dev)
d_of = torch.arange(A, dtype=torch.int32, device=dev).repeat_interleave(I).contiguous()
d_idx = torch.arange(I, dtype=torch.int32, device=dev).repeat(A).contiguous()
d_row = torch.arange(I, dtype=torch.int32, device=dev)
n = A * I
one = [u8(32 * n), u8(96 * n), u8(48 * n), u8(4 * n)]
loop = [u8(32 * n), u8(96 * n), u8(48 * n)]


def grid_one():
    eng.hd_paths_dev(d_par.data_ptr(), A, False, d_of.data_ptr(), d_idx.data_ptr(), 1, n, one[0].data_ptr(), None, one[1].data_ptr(),
                     one[2].data_ptr(), one[3].data_ptr(), st.cuda_stream)


def grid_loop():
    for a in range(A):
        eng.hd_children_dev(acc_chain[32 * a:32 * a + 32], acc_aff[96 * a:96 * a + 96], None, d_row.data_ptr(), I,
                            loop[0].data_ptr() + 32 * I * a, None, loop[1].data_ptr() + 96 * I * a, loop[2].data_ptr() + 48 * I * a,
                            st.cuda_stream)


t_one, t_loop = alternate(grid_one, grid_loop)
same = all(bool(torch.equal(x, y)) for x, y in zip(one[:3], loop))
log("%12s %16s %8s %s" % ("hd_paths ms", "256 calls ms", "ratio", "outputs equal"))
log("%12.3f %16.3f %8.1f %s" % (t_one, t_loop, t_loop / t_one, same))
d_idx2 = torch.stack([d_of, d_idx], dim=1).contiguous()
d_root = torch.frombuffer(bytearray(root_chain + G + bytes(32)), dtype=torch.uint8).to(dev)
two = [u8(32 * n), u8(96 * n), u8(48 * n), u8(4 * n)]


def grid_two():
    eng.hd_paths_dev(d_root.data_ptr(), 1, False, None, d_idx2.data_ptr(), 2, n, two[0].data_ptr(), None, two[1].data_ptr(), two[2].data_ptr(),
                     two[3].data_ptr(), st.cuda_stream)


for _ in range(2):
    timed(grid_two)
t_two = statistics.median(timed(grid_two) for _ in range(reps))
log("the same leaves as 65 536 paths of depth 2 from the root (the account level derived 256 times over): %.3f ms, outputs equal %s"
    % (t_two, all(bool(torch.equal(x, y)) for x, y in zip(one, two))))
del one, loop, two, d_of, d_idx, d_idx2
torch.cuda.empty_cache()

log("\n## 2. private paths m/h/h/a/i of depth 4 (hardened, hardened, not, not): one call vs per-parent calls level by level")
log("   (per-parent figure: hd_children_dev calls timed on a sample of prefixes of each level, SCALED to the level's distinct prefixes)")
log("%9s %12s %14s %22s %8s" % ("n", "hd_paths ms", "paths/s", "per-parent ms (scaled)", "ratio"))
sk = (12345).to_bytes(32, "big")
d_prv = torch.frombuffer(bytearray(root_chain + G + sk), dtype=torch.uint8).to(dev)
SAMPLE = 32
for n, shape in ((65536, (4, 16, 32, 32)), (1 << 20, (4, 16, 128, 128))):
    h0, h1, na, ni = shape
    p = torch.arange(n, dtype=torch.int64, device=dev)
    cols = [(p // (h1 * na * ni)) - H31, (p // (na * ni)) % h1 - H31, (p // ni) % na, p % ni]    # (x - 2^31 is 2^31 + x as uint32)
    d_idx = torch.stack(cols, dim=1).to(torch.int32).contiguous()
    outs = [u8(32 * n), u8(32 * n), u8(96 * n), u8(48 * n), u8(4 * n)]

    def paths_one():
        eng.hd_paths_dev(d_prv.data_ptr(), 1, True, None, d_idx.data_ptr(), 4, n, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                         outs[3].data_ptr(), outs[4].data_ptr(), st.cuda_stream)

    # level l: `calls` distinct prefixes, each one hd_children_dev call of `width` children
    levels = [(1, h0, True), (h0, h1, True), (h0 * h1, na, False), (h0 * h1 * na, ni, False)]
    widest = max(w for _, w, _ in levels)
    d_lvl = torch.arange(widest, dtype=torch.int32, device=dev)
    d_lvl_h = (torch.arange(widest, dtype=torch.int64, device=dev) - H31).to(torch.int32)     # 2^31 + i as uint32
    lv = [u8(32 * widest), u8(32 * widest), u8(96 * widest), u8(48 * widest)]
    scaled = 0.0
    t_one = None
    for calls, width, hard in levels:
        m = min(calls, SAMPLE)

        def level_calls():
            for _ in range(m):
                eng.hd_children_dev(root_chain, G, sk, (d_lvl_h if hard else d_lvl).data_ptr(), width, lv[0].data_ptr(), lv[1].data_ptr(),
                                    lv[2].data_ptr(), lv[3].data_ptr(), st.cuda_stream)

        t_one, t_lvl = alternate(paths_one, level_calls)
        scaled += t_lvl * calls / m
    log("%9d %12.3f %14.3e %22.1f %8.1f" % (n, t_one, n / (t_one / 1e3), scaled, scaled / t_one))
    del d_idx, outs, p, cols
    torch.cuda.empty_cache()

log("\n## 3. depth 1, one parent: hd_paths_dev vs hd_children_dev on the same indices (the cost of per-lane midstates), alternating")
log("%9s %8s %12s %16s %8s %s" % ("n", "mode", "hd_paths ms", "hd_children ms", "ratio", "outputs equal"))
for n in (1, 65536, 1 << 20):
    d_idx = torch.arange(n, dtype=torch.int32, device=dev)
    a = [u8(32 * n), u8(32 * n), u8(96 * n), u8(48 * n), u8(4 * n)]
    b = [u8(32 * n), u8(32 * n), u8(96 * n), u8(48 * n)]
    for mode, psk, d_rec in (("public", None, d_root), ("private", sk, d_prv)):
        f = lambda: eng.hd_paths_dev(d_rec.data_ptr(), 1, psk is not None, None, d_idx.data_ptr(), 1, n, a[0].data_ptr(), a[1].data_ptr(),
                                     a[2].data_ptr(), a[3].data_ptr(), a[4].data_ptr(), st.cuda_stream)
        g = lambda: eng.hd_children_dev(root_chain, G, psk, d_idx.data_ptr(), n, b[0].data_ptr(), b[1].data_ptr() if psk else None,
                                        b[2].data_ptr(), b[3].data_ptr(), st.cuda_stream)
        tf, tg = alternate(f, g)
        same = all(bool(torch.equal(a[o], b[o])) for o in ((0, 1, 2, 3) if psk else (0, 2, 3)))
        log("%9d %8s %12.3f %16.3f %8.2f %s" % (n, mode, tf, tg, tf / tg, same))
    del d_idx, a, b
    torch.cuda.empty_cache()

log("\n## 4. ExtendedPublicKey.public_paths_from for the 256 x 256 grid, Python end to end (host clock)")
from bls_py.keys import ExtendedPrivateKey, ExtendedPublicKey  # noqa: E402
xpub = ExtendedPrivateKey.from_seed(b"hd_paths_probe").get_extended_public_key()
accounts = xpub.public_child_batch(range(A))
parent_of = [a for a in range(A) for _ in range(I)]
paths = [[i] for _ in range(A) for i in range(I)]
ExtendedPublicKey.public_paths_from(accounts, parent_of[:64], paths[:64])
ts = []
for _ in range(3):
    t0 = time.perf_counter()
    leaves = ExtendedPublicKey.public_paths_from(accounts, parent_of, paths)
    ts.append((time.perf_counter() - t0) * 1e3)
t0 = time.perf_counter()
rows = [acc.public_child_batch(range(I)) for acc in accounts]
t_rows = (time.perf_counter() - t0) * 1e3
log("65536 leaves: %.1f ms median of 3 (%.2f us per leaf); 256 public_child_batch calls: %.1f ms; leaves equal: %s"
    % (statistics.median(ts), statistics.median(ts) * 1e3 / (A * I), t_rows,
       [k.serialize() for k in leaves] == [k.serialize() for r in rows for k in r]))

os.makedirs(out_dir, exist_ok=True)
with open(os.path.join(out_dir, "hd_paths_probe.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
eng.close()
