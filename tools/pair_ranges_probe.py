"""The ragged multi-pairing (csrc/blsgpu_mlr.hip) against the loop it would replace: blsgpu_pairing_multi_ranges_dev over one
pair list against one blsgpu_pairing_multi_batch_dev per size class over the same pairs (ranges of one length lie side by side,
so both read the list as it is).  Medians of 3 calls after one warm-up call, _dev forms, device events, all in one run:
  (a) 1000 ranges of lengths 2 .. 201 (five of each): 200 size classes;
  (b) 32 768 ranges of 2;
  (c) 10 000 ranges of 5;
  (d) one range of 1024 + 1024 ranges of 2.
Each with the chunk C = BLSGPU_PAIR_RANGES_CHUNK in 8, 16 (the default), 32, 64 -- a context per value.  No ratio is fixed in
advance: whatever comes out is recorded, a loss included; BLS.verify_batch stays unrouted, and whoever routes it quotes this file.
usage: python3 tools/pair_ranges_probe.py [out_dir (default profiles)]
Writes <out_dir>/pair_ranges_probe.txt, stamped with the library's version string and a digest of libblsgpu.so."""
import hashlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "python-bls_amd"))
REPS = 3
CHUNKS = (8, 16, 32, 64)


def engine_with_chunk(C):
    from bls_py import _native
    old = os.environ.get("BLSGPU_PAIR_RANGES_CHUNK")
    os.environ["BLSGPU_PAIR_RANGES_CHUNK"] = str(C)
    try:
        return _native.Engine(0)
    finally:
        if old is None:
            del os.environ["BLSGPU_PAIR_RANGES_CHUNK"]
        else:
            os.environ["BLSGPU_PAIR_RANGES_CHUNK"] = old


def shapes():
    """(label, [(length, how many)] in the order the ranges lie in the pair list)"""
    return [("(a) 1000 ranges of lengths 2 .. 201", [(v, 5) for v in range(2, 202)]),
            ("(b) 32768 ranges of 2", [(2, 32768)]),
            ("(c) 10000 ranges of 5", [(5, 10000)]),
            ("(d) 1 range of 1024 + 1024 ranges of 2", [(1024, 1), (2, 1024)])]


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles")

    import torch
    from bls_py import _native
    from bls_py import _native_pairranges as R

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

    def measure(fns):
        for f in fns:
            timed(f)
        ts = [[] for _ in fns]
        for _ in range(REPS):
            for t, f in zip(ts, fns):
                t.append(timed(f))
        return ts

    with open(os.path.join(ROOT, "tests", "golden", "pairs_seed1_g1.bin"), "rb") as f:
        g1 = f.read()
    with open(os.path.join(ROOT, "tests", "golden", "pairs_seed1_g2.bin"), "rb") as f:
        g2 = f.read()
    top = max(sum(v * k for v, k in cls) for _, cls in shapes())
    reps = -(-top // 1025)
    d_g1 = torch.frombuffer(bytearray((g1 * reps)[:96 * top]), dtype=torch.uint8).to(dev)     # the 1025 seeded pairs, over and over
    d_g2 = torch.frombuffer(bytearray((g2 * reps)[:192 * top]), dtype=torch.uint8).to(dev)

    engines = {C: engine_with_chunk(C) for C in CHUNKS}
    eng = engines[16]
    with open(os.environ.get("BLSGPU_LIBRARY", _native._LIB_PATH), "rb") as f:
        lib_digest = hashlib.sha256(f.read()).hexdigest()[:16]
    log("# pair_ranges_probe: %s sha256 %s, %s, medians of %d calls after 1 warm-up call (median, min, max), device events, ms"
        % (eng.version(), lib_digest, torch.cuda.get_device_name(0), REPS))

    for label, classes in shapes():
        ranges, at = [], 0
        for v, k in classes:
            for _ in range(k):
                ranges.append((at, at + v))
                at += v
        n, m = at, len(ranges)
        d_a = torch.zeros(576 * m, dtype=torch.uint8, device=dev)
        d_b = torch.zeros(576 * m, dtype=torch.uint8, device=dev)

        tab, _ = R.range_table(eng, ranges)                   # marshalled once: the library's own host plan stays inside the timed call

        def ragged(e, d_out=d_a):
            return lambda: e._call("blsgpu_pairing_multi_ranges_dev", d_g1.data_ptr(), d_g2.data_ptr(), None, n, tab, m, d_out.data_ptr(),
                                   st.cuda_stream)

        def per_class():
            pair, res = 0, 0
            for v, k in classes:
                eng.pairing_multi_batch_dev(d_g1.data_ptr() + 96 * pair, d_g2.data_ptr() + 192 * pair, v, k, d_b.data_ptr() + 576 * res,
                                            stream=st.cuda_stream)
                pair, res = pair + v * k, res + k
        ts = measure([per_class] + [ragged(engines[C]) for C in CHUNKS])
        base = statistics.median(ts[0])
        log("\n## %s: %d pairs, %d ranges, %d size classes" % (label, n, m, len(classes)))
        log("per-class loop of pairing_multi_batch_dev (%d calls) %s" % (len(classes), spread(ts[0])))
        for C, t in zip(CHUNKS, ts[1:]):
            timed(ragged(engines[C]))
            same = bool(torch.equal(d_a, d_b))
            log("pairing_multi_ranges_dev, C = %2d                  %s   ragged / per-class %.3f   same bytes: %s"
                % (C, spread(t), statistics.median(t) / base, same))
        del d_a, d_b

    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "pair_ranges_probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    for e in engines.values():
        e.close()


if __name__ == "__main__":
    main()
