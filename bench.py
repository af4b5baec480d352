#!/usr/bin/env python3
"""bench.py -- BLS12-381 pairings/sec through the HIP multi-pairing engine.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config c2|c3|c4|c5|h2c] [--full] [--dump-outputs DIR]

A plain c2 / c3 run sets up, warms up, times the K steps and prints the line; --full adds the result checks and every
other figure (multiply-add probe, clock samples, single-call latencies, c3's 8-GPU projection, CPU baselines, and after
c2 the secondary configs).  --dump-outputs DIR writes the results of the last timed step (DIR/pairings.npy: B x 12 x 48
bytes as float32, one Fq12 per verification); the inputs are PRF-seeded, the same in every run with the same arguments.

With --gpus N > 1 and no WORLD_SIZE in the environment the script starts itself under
`python -m torch.distributed.run` as a CHILD process (before anything touches a GPU) and
exits with the child's code; under an external torchrun it just reads RANK / WORLD_SIZE.

A "step" is one pass of the hot path over one batch already resident in HBM.

  c2 (default, headline; BASELINE.json configs[1] shape x 512, weak scaling)
      B = 512 independent aggregate verifications per step (round 3; 32 in rounds 1-2: a step of 32 800 pairs lasted 6 ms, so
      the driver's 20 steps were a 0.13 s timed region.  The line-stream kernels run 16 400 + 33 000 wavefronts per
      step at B = 512: the last, partly filled round of wavefronts costs 6 % of a step, 12 % at B = 256 -- measured
      12.65 against 11.84 M pairings/s), each fq_ate_pairing_multi over 1025
      (pk, H(m)) pairs per GPU (1024 signatures + the (-G1, aggregate) pair): Miller loops,
      Fq12 products, B final exponentiations.  The 512 x 1025 pairs of a rank are 524 800 DIFFERENT
      PRF-seeded points; verification 0 on rank 0 is the batch whose result the
      reference produced (tests/golden/pairing.json).  N ranks: Miller products per rank, ONE RCCL
      all-gather of B x 576 bytes per rank, the B final exponentiations on every rank.
  c3  (BASELINE configs[2]; strong scaling) ONE multi-pairing of 65 536 pairs, sharded N ways
      (8 192 per GPU at N = 8): one Miller product per rank, all-gather of one 576-byte partial
      per rank, one final exponentiation on every rank.
  c4  threshold k = 67 of n = 100: 10 000 combines (G2 multi-scalar sums) + 10 000 two-pair verifies per GPU.
  c5  ONE G1 multi-scalar sum over 2^20 different points (aggregate_pub_keys, secure = True), the points split over the
      ranks (strong scaling): per-rank sum, all-gather of one 100-byte record per rank, `world` additions.
  h2c hash 16 384 message hashes to G2.

Every configuration (c2 / c3 with --full) checks its results (reference golden vectors where they exist, bilinearity /
linearity identities evaluated by the engine itself otherwise) and aborts on a mismatch.
Prints ONE JSON line on rank 0.
"""
import argparse
import contextlib
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "python-bls_amd"))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

PAIRS_PER_GPU = 1025
VERIFICATIONS_PER_STEP = 512
C3_PAIRS = 65536
# algorithmic work, SURVEY.md section 8(d): 6754 Fq-mults per pairing at 300 32-bit MACs each,
# ~9.5k Fq-mults per final exponentiation; G2 / G1 mixed additions at 36 / 11 Fq-mults
MAC_PER_FQ_MUL = 300
MAC_PER_PAIRING = 6754 * MAC_PER_FQ_MUL
MAC_PER_FINAL_EXP = 9500 * MAC_PER_FQ_MUL
HBM_BYTES_PER_PAIRING = 288
PEAK_TMACS = 34.65        # measured v_mad_u64_u32 rate, profiles/r01_intrate_microbench.txt
PEAK_HBM_GBS = 8000.0
# line-stream Miller stage (csrc/blsgpu_ml.hip): 68 line records of 336 bytes per pair, written once and read once
LS_LINES = 68
LS_LINE_BYTES_PER_PAIRING = LS_LINES * 336
PEAK_MAD28_T = 34.1       # measured v_mad_i64_i32 rate, profiles/r03_fp28_microbench.txt
DUMP_LIMIT_BYTES = 64 << 20
N_ORDER = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def prf_scalar(tag, seed, i):
    """counter-mode PRF scalar in [1, n-1] (same as tests/golden/make_golden.py)."""
    h = hashlib.sha256(tag + seed.to_bytes(4, "big") + i.to_bytes(4, "big"))
    return int.from_bytes(h.digest(), "big") % (N_ORDER - 1) + 1


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@contextlib.contextmanager
def stdout_to_stderr():
    """file descriptor 1 -> 2 for the duration (native libraries write there directly)"""
    sys.stdout.flush()
    keep = os.dup(1)
    os.dup2(2, 1)
    try:
        yield
    finally:
        os.dup2(keep, 1)
        os.close(keep)


def self_launch(args):
    """--gpus N without a launcher: run this script under torch.distributed.run as a child (this
    process has not touched a GPU) and hand its exit code on."""
    port = free_port()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.run(cmd, env=env).returncode


def source_hash():
    """sha256 (16 hex digits) over the kernel sources the loaded library was built from"""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "python-bls_amd", "csrc")
    for name in sorted(os.listdir(d)):
        if name.endswith((".hip", ".h")):
            with open(os.path.join(d, name), "rb") as f:
                h.update(name.encode() + b"\0" + f.read())
    return h.hexdigest()[:16]


def pmc_traffic(kernels, pairings_per_launch):
    """HBM bytes per launch of the Miller-stage kernels from the COMMITTED rocprofv3 --pmc passes (FETCH_SIZE and
    WRITE_SIZE, KB per dispatch, separate passes; tools/ml_pmc.sh on this same workload).  Counters cannot be read
    inside this process, so the figure is reported only when the summary's header names THIS build (source hash) and
    this launch size; FETCH_SIZE is doubled as MI355X_MICROARCH.md prescribes for 16-byte-per-lane streaming reads."""
    import glob
    cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_ls_pmc_summary.csv")))
    if not cands:
        return None, None
    path = cands[-1]                                     # the latest round's passes; used only if its header names this build
    kb, ok = {}, False
    with open(path) as f:
        for row in f:
            if row.startswith("#"):
                ok = ("build " + source_hash()) in row and ("pairs %d" % pairings_per_launch) in row
                continue
            c = row.strip().split(",")
            if len(c) == 4 and c[0].split("::")[-1].replace("k_ml_lines2", "k_ml_lines").replace("k_ml_horner_wide", "k_ml_horner").replace("k_ml_horner_fexp", "k_ml_horner").replace("k_ml_merge_wide", "k_ml_merge") in kernels and c[1] in ("FETCH_SIZE", "WRITE_SIZE"):
                kb[(c[0].split("::")[-1], c[1])] = float(c[3])
    if not ok or not kb:
        return None, None
    total = sum(v * (2 if k[1] == "FETCH_SIZE" else 1) for k, v in kb.items()) * 1024
    return int(total), "profiles/" + os.path.basename(path)


def config_traffic(name):
    """HBM bytes per step of a secondary config (c4 / c5 / h2c) from the COMMITTED rocprofv3 --pmc passes over `bench.py --config
    <name>` (tools/profile_round.sh; tools/collect_profiles.py sums FETCH_SIZE and WRITE_SIZE of the dispatches between the timed
    region's marks, per step) -- reported only when the summary's header names THIS build; FETCH_SIZE doubled as for pmc_traffic."""
    import glob
    cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_configs_traffic.csv")))
    if not cands:
        return None, None
    path, ok, kb = cands[-1], False, {}
    with open(path) as f:
        for row in f:
            if row.startswith("#"):
                ok = ("build " + source_hash()) in row
                continue
            c = row.strip().split(",")
            if len(c) == 4 and c[0] == name and c[1] in ("FETCH_SIZE", "WRITE_SIZE"):
                kb[c[1]] = float(c[3])
    if not ok or len(kb) != 2:
        return None, None
    return int((2 * kb["FETCH_SIZE"] + kb["WRITE_SIZE"]) * 1024), "profiles/" + os.path.basename(path)


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for ln in f:
                if ln.startswith("model name"):
                    return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def usable_cores():
    """host threads this process may actually run on: affinity mask and cgroup CPU quota (a GPU box
    hands a container a share of the host, os.cpu_count() reports the whole machine)"""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()
        if quota != "max":
            n = min(n, max(1, int(quota) // int(period)))
    except (OSError, ValueError):
        pass
    return n


def cpu_baseline(g1, g2, n, gpu_out):
    """The oracle (CPU restatement of the reference's algorithm: affine lines with an Fq12 inversion
    per step, 1268-bit final exponentiation) on THIS box's host cores, bounded sample (about 10-20 s
    of CPU work): one thread on 512 pairs, then every usable core on eight copies of the 1025-pair
    batch.  The all-core result is compared with the GPU's (its 8th power)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as O
    O.build()
    cores = usable_cores()
    n1 = min(512, n)
    t = time.perf_counter()
    O.pairing_multi(g1[:96 * n1], g2[:192 * n1], n1, threads=1)
    d1 = time.perf_counter() - t
    copies = 8
    t = time.perf_counter()
    out = O.pairing_multi(g1 * copies, g2 * copies, copies * n, threads=cores)
    dt = time.perf_counter() - t
    ok = gpu_out is None or out == O.fq12_pow(gpu_out, copies)
    # the FAST-ALGORITHM flavour: projective twist point, sparse lines, one shared squaring per thread --
    # the algorithm of the GPU path on the host cores (oracle.pairing_multi_fast; ordinary pairs only)
    t = time.perf_counter()
    f1 = O.pairing_multi_fast(g1[:96 * n], g2[:192 * n], n, 1)
    df1 = time.perf_counter() - t
    fcopies = 32
    t = time.perf_counter()
    fout = O.pairing_multi_fast(g1 * fcopies, g2 * fcopies, fcopies * n, cores)
    dfa = time.perf_counter() - t
    ok = ok and (gpu_out is None or (f1 == gpu_out and fout == O.fq12_pow(gpu_out, fcopies)))
    fast = {"value": fcopies * n / dfa, "unit": "pairings/s", "cores": cores, "kind": "port",
            "algorithm": "projective twist point, sparse lines, shared squaring (the GPU path's algorithm on the CPU)",
            "sample": "%d copies of the %d-pair batch on %d threads, %.2f s wall" % (fcopies, n, cores, dfa),
            "single_thread": {"value": n / df1, "unit": "pairings/s", "cores": 1,
                              "sample": "%d pairs + one final exponentiation, %.2f s wall" % (n, df1)}}
    return {"value": copies * n / dt, "fast_algorithm": fast, "unit": "pairings/s", "cores": cores, "kind": "port", "cpu_model": cpu_model(),
            "host_logical_cpus": os.cpu_count(),
            "sample": "%d copies of the %d-pair batch on %d threads, %.2f s wall" % (copies, n, cores, dt),
            "single_thread": {"value": n1 / d1, "unit": "pairings/s", "cores": 1,
                              "sample": "%d pairs + one final exponentiation, %.2f s wall" % (n1, d1)},
            "reference_measured_in_build_container": "BASELINE.md: native Cython+GMP 259 pairings/s, pure Python 24-33 pairings/s, 1 core",
            "matches_gpu": ok}


class Env:
    """process group, device, engine streams"""

    def __init__(self, args):
        import torch
        self.torch = torch
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        local = int(os.environ.get("LOCAL_RANK", "0"))
        ndev = torch.cuda.device_count()
        self.local_dev = local % max(1, ndev)
        torch.cuda.set_device(self.local_dev)
        self.dev = torch.device("cuda", self.local_dev)
        self.dist = None
        self.clock = None
        self.backend = args.backend
        if self.world > 1 or args.force_process_group:
            import torch.distributed as dist
            self.dist = dist
            if "MASTER_ADDR" not in os.environ:                # a forced one-rank group started without a launcher
                os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), RANK="0", WORLD_SIZE="1")
            # librccl (a version banner) and gloo (its connection report) print on stdout when the group forms:
            # send that to stderr, stdout carries the one JSON line only
            with stdout_to_stderr():
                if args.backend == "nccl":
                    dist.init_process_group("nccl", device_id=self.dev)
                    dist.barrier()
                    torch.cuda.synchronize()
                else:
                    dist.init_process_group("gloo")
                    dist.barrier()
            assert dist.get_world_size() == max(1, self.world)

    def up(self, b):
        return self.torch.frombuffer(bytearray(b), dtype=self.torch.uint8).to(self.dev)

    def barrier(self):
        self.torch.cuda.synchronize()
        if self.dist:
            self.dist.barrier()
        self.torch.cuda.synchronize()

    def max_over_ranks(self, x):
        if not self.dist:
            return x
        t = self.torch.tensor([x], dtype=self.torch.float64, device=self.dev if self.backend == "nccl" else "cpu")
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def gather_objects(self, obj):
        if not self.dist:
            return [obj]
        out = [None] * self.world
        self.dist.all_gather_object(out, obj)
        return out

    def all_gather_partials(self, stream, src, dst, words):
        """one all-gather of `words` int32 per rank (RCCL; gloo = rehearsal through host memory)"""
        torch = self.torch
        with torch.cuda.stream(stream):
            if self.backend == "nccl":
                self.dist.all_gather_into_tensor(dst, src)
            else:
                stream.synchronize()
                host = [torch.zeros(words, dtype=torch.int32) for _ in range(self.world)]
                self.dist.all_gather(host, src.cpu())
                dst.copy_(torch.cat(host).to(self.dev))

    def finish(self):
        if self.dist:
            self.dist.barrier()
            self.dist.destroy_process_group()


def seeded_points(eng, gen1, gen2, idx):
    """P_i = a_i G1, Q_i = b_i G2 for the PRF indices idx (seed 1), computed with the engine's own
    group sums (k = 1 per group); returns (g1 bytes, g2 bytes, a, b)."""
    a = [prf_scalar(b"blsgpu/a", 1, i) for i in idx]
    b = [prf_scalar(b"blsgpu/b", 1, i) for i in idx]
    m = len(idx)
    g1, _ = eng.g1_msm(gen1 * m, a, 1, m)
    g2, _ = eng.g2_msm(gen2 * m, b, 1, m)
    return g1, g2, a, b


class ClockWatch:
    """Engine clock and package power of this rank's GPU while the timed steps run: the hwmon files of the card whose PCI
    address torch reports (freq1_input in Hz, power1_input in uW), read every 50 ms by a thread -- sysfs reads only, no
    child process.  The roof this bench prices against is a power-limited one ("Clock and power"),
    so the line carries the clock the step ran at."""

    def __init__(self, torch, index):
        import glob
        self.files, self.samples, self._stop, self._t = None, [], False, None
        try:
            pr = torch.cuda.get_device_properties(index)
            addr = "%04x:%02x:%02x.0" % (pr.pci_domain_id, pr.pci_bus_id, pr.pci_device_id)
            for d in glob.glob("/sys/class/drm/card*/device"):
                if os.path.realpath(d).endswith(addr):
                    f = glob.glob(os.path.join(d, "hwmon", "hwmon*", "freq1_input"))
                    w = glob.glob(os.path.join(d, "hwmon", "hwmon*", "power1_input")) or glob.glob(os.path.join(d, "hwmon", "hwmon*", "power1_average"))
                    if f:
                        self.files = (f[0], w[0] if w else None)
        except Exception:
            self.files = None

    def _run(self):
        while not self._stop:
            try:
                with open(self.files[0]) as f:
                    hz = int(f.read().split()[0])
                uw = None
                if self.files[1]:
                    with open(self.files[1]) as f:
                        uw = int(f.read().split()[0])
                self.samples.append((hz / 1e6, None if uw is None else uw / 1e6))
            except (OSError, ValueError, IndexError):
                pass
            time.sleep(0.05)

    def start(self):
        if self.files:
            import threading
            self._t = threading.Thread(target=self._run, daemon=True)
            self._t.start()

    def stop(self):
        self._stop = True
        if self._t:
            self._t.join(timeout=1.0)
        mhz = sorted(s[0] for s in self.samples)
        wat = sorted(s[1] for s in self.samples if s[1] is not None)
        if not mhz:
            return None
        return {"sclk_mhz_median": mhz[len(mhz) // 2], "sclk_mhz_min": mhz[0], "sclk_mhz_max": mhz[-1],
                "package_power_w_median": wat[len(wat) // 2] if wat else None, "samples": len(mhz)}


def timed_steps(env, args, step, engs, streams):
    """W warm-up steps, [--full: the multiply-add probe,] barrier, K timed steps, barrier: (seconds max over ranks, per-step ms,
    kernel times)"""
    torch = env.torch
    S = len(streams)
    torch.cuda.synchronize()
    for i in range(args.warmup):
        step(i)
    torch.cuda.synchronize()
    # the roof in THIS process on THIS box: ~30 ms of v_mad_i64_i32 on every SIMD right before the timed steps (the chip is warm
    # and at its power-limited clock after the warm-up steps)
    env.peak_now = engs[0].mad_probe(30.0) if args.full and not args.no_peak_probe else None
    env.barrier()
    for e in engs:
        e.timing_enable(True)         # HIP events around every kernel, on the stream it runs on
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    watch = ClockWatch(torch, env.local_dev) if args.full else None
    if watch:
        watch.start()
    engs[0].mark(1)                   # (the device is idle here: everything dispatched until the closing mark is the timed region)
    t0 = time.perf_counter()
    for i in range(args.steps):
        ev[i][0].record(streams[i % S])
        step(i)
        ev[i][1].record(streams[i % S])
    env.barrier()
    dt = env.max_over_ranks(time.perf_counter() - t0)
    engs[0].mark(2)
    env.clock = watch.stop() if watch else None
    step_ms = sorted(a.elapsed_time(b) for a, b in ev)
    ktimes = [t for e in engs for t in e.timing_read()]
    for e in engs:
        e.timing_enable(False)
    return dt, step_ms, ktimes


def bilinear_expectation(eng, gen1, gen2, sums):
    """e(G1, G2)^s for every s in sums, as the engine's pairing of (s G1, G2): the check of SURVEY 8c
    (prod e(a_i G1, b_i G2) = e(G1, G2)^(sum a_i b_i)), independent of any oracle."""
    m = len(sums)
    pts, _ = eng.g1_msm(gen1 * m, [s % N_ORDER for s in sums], 1, m)
    out = eng.pairing_multi_batch(pts, gen2 * m, 1, m)
    return [out[576 * i:576 * (i + 1)] for i in range(m)]


def latency_probe(env, eng, t1, t2, n, stream, reps=4):
    torch = env.torch
    out = torch.zeros(576, dtype=torch.uint8, device=env.dev)
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        eng.pairing_multi_dev(t1.data_ptr(), t2.data_ptr(), n, out.data_ptr(), stream.cuda_stream)
        b.record(stream)
        stream.synchronize()
        ms.append(a.elapsed_time(b))
    return min(ms)


def dump_outputs(d, arrays, limit=DUMP_LIMIT_BYTES):
    """--dump-outputs: each tensor as d/<name>.npy in float32 (its byte values are exact there).  One beyond its share of
    `limit` keeps a fixed, seeded sample of its rows (first axis), their indices in d/<name>_rows.npy."""
    import numpy as np
    os.makedirs(d, exist_ok=True)
    share = limit // len(arrays)
    for name, t in arrays.items():
        a = t.cpu().numpy().astype(np.float32)
        if a.nbytes > share:
            row = a.nbytes // a.shape[0]
            rows = np.sort(np.random.default_rng(0).choice(a.shape[0], share // (row + 8), replace=False))
            np.save(os.path.join(d, name + "_rows.npy"), rows.astype(np.float64))
            a = a[rows]
        np.save(os.path.join(d, name + ".npy"), a)


def run_pairing(env, args):
    torch = env.torch
    from bls_py import _native
    world, rank, dev = env.world, env.rank, env.dev
    c3 = args.config == "c3"
    S = max(1, args.streams)
    engs = [_native.Engine(env.local_dev) for _ in range(S)]
    eng = engs[0]
    gold = os.path.join(ROOT, "tests", "golden")
    with open(os.path.join(gold, "pairing.json")) as f:
        gj = json.load(f)
    gen1, gen2 = bytes.fromhex(gj["gen"]["g1"]), bytes.fromhex(gj["gen"]["g2"])
    if c3:
        total = args.pairs_total
        lo, hi = total * rank // world, total * (rank + 1) // world
        n, B = hi - lo, 1
        idx = list(range(lo, hi))                       # rank r holds pairs [lo, hi) of the ONE verification
    else:
        n, B = args.pairs, max(1, args.verifications)
        # verification v of rank r: PRF indices ((v * world + r) * n ...): all different; v = 0 on rank 0
        # is the batch of tests/golden/pairing.json "seeded"
        idx = [((v * world + rank) * n + j) for v in range(B) for j in range(n)]
    g1, g2, a, b = seeded_points(eng, gen1, gen2, idx)
    t1, t2 = env.up(g1), env.up(g2)
    outs = [torch.zeros(B * 576, dtype=torch.uint8, device=dev) for _ in range(S)]
    parts = [torch.zeros(B * 144, dtype=torch.int32, device=dev) for _ in range(S)]
    gath = [torch.zeros(world * B * 144, dtype=torch.int32, device=dev) for _ in range(S)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(S)]
    for e in engs:
        e.reserve((n + 3) * B)
        e.set_mp_threshold(0 if n * B >= 2048 else 1 << 40)    # throughput kernel once the batch can fill the GPU
    from bls_py.dist import GpuShardBackend                    # the product's own multi-GPU class does the steps
    shard = [GpuShardBackend(e, dev) for e in engs]

    # A step = Miller loops + per-verification products (stream k), [all-gather,] then the B final
    # exponentiations.  Miller launches of consecutive steps are serialised with an event (they would
    # only stretch each other), so the final exponentiations of step i (B wavefronts, latency bound)
    # overlap the Miller loops of step i + 1.
    # The order is kept with the engine's "bulk" event (blsgpu_ctx_set_bulk_event): recorded right after the last
    # chip-filling kernel of the stage, so the few dozen wavefronts of Horner / products / final exponentiations of
    # step i run beside the point chains of step i + 1.
    bulk = [torch.cuda.Event() for _ in range(S)]
    for k in range(S):
        bulk[k].record(streams[k])                   # creates the HIP event behind the torch object
        engs[k].set_bulk_event(bulk[k].cuda_event)
    torch.cuda.synchronize()
    miller_done = [None]

    def step(i):
        k = i % S
        stream = streams[k]
        st = stream.cuda_stream
        if miller_done[0] is not None and not args.free_streams:
            stream.wait_event(miller_done[0])
        shard[k].miller_partials_batch_dev(t1, t2, n, B, parts[k], st)
        miller_done[0] = bulk[k]
        if env.dist is None:
            shard[k].final_batch_dev(parts[k], 1, B, outs[k], st)
        else:
            if env.backend == "nccl":
                with torch.cuda.stream(stream):
                    shard[k].all_gather_into(gath[k], parts[k])             # RCCL: B x 576 bytes per rank
            else:
                env.all_gather_partials(stream, parts[k], gath[k], B * 144)  # gloo rehearsal through host memory
            shard[k].final_batch_dev(gath[k], world, B, outs[k], st)

    dt, step_ms, ktimes = timed_steps(env, args, step, engs, streams)
    if args.dump_outputs and rank == 0:
        # what the caller of the step receives: B Fq12 values of 12 coefficients, 48 big-endian bytes each (every rank holds them)
        dump_outputs(args.dump_outputs, {"pairings": outs[(args.steps - 1) % S].view(B, 12, 48)})
    ws_after_steps = {"all_contexts": sum(e.workspace_bytes()["total"] for e in engs), "contexts": len(engs), "one_context": eng.workspace_bytes()}
    full = args.full
    if full:
        results = [bytes(o.cpu().numpy()) for o in outs[:min(S, args.steps)]]
        assert all(r == results[0] for r in results), "streams disagree"
        per = [results[0][576 * v:576 * (v + 1)] for v in range(B)]
    miller_ms = [ms for k, ms in ktimes if k == 0]
    reduce_ms = [ms for k, ms in ktimes if k == 1]
    fexp_ms = [ms for k, ms in ktimes if k == 2]
    slow_ms = [ms for k, ms in ktimes if k == 3]
    # line-stream Miller stage (csrc/blsgpu_ml.hip): kinds 4 k_ml_lines, 5 k_ml_accum, 6 k_ml_merge, 7 k_ml_horner;
    # one k_ml_lines launch per step
    ls = {name: [ms for k, ms in ktimes if k == kind] for kind, name in
          ((4, "k_ml_lines"), (5, "k_ml_accum"), (6, "k_ml_merge"), (7, "k_ml_horner"))}
    line_stream = bool(ls["k_ml_lines"])
    if line_stream:
        launches = args.steps                        # per STEP (a step of more than 2^20 pairs is several launch sequences)
        ls_avg = {name: sum(v) / launches for name, v in ls.items()}
        miller_avg = sum(ls_avg.values())
    else:
        launches = len(miller_ms)
        miller_avg = sum(miller_ms) / len(miller_ms)
    # every rank's sums of a_i b_i per verification (--full: for the check) and its kernel time go to rank 0
    sums = [sum(x * y for x, y in zip(a[v * n:(v + 1) * n], b[v * n:(v + 1) * n])) % N_ORDER for v in range(B)] if full else None
    info = env.gather_objects({"rank": rank, "sums": sums, "k_miller_ms_avg": miller_avg, "pairs": n * B,
                               "device": torch.cuda.get_device_name(dev)})
    # latency views of the literal configs on this GPU alone: one 1025-pair verification, one 8192-pair shard
    # ONE step alone on an idle GPU with the kernel timers on: the durations of the few-wavefront kernels (products of
    # partials, Horner, final exponentiations) as they are, not stretched by the next step's chip-filling point chains
    solo = {}
    if full and rank == 0 and env.dist is None:
        torch.cuda.synchronize()
        eng.timing_enable(True)
        step(0)
        torch.cuda.synchronize()
        kt = eng.timing_read()
        eng.timing_enable(False)
        names = {0: "k_miller", 1: "k_reduce", 2: "final_exp", 3: "k_ml_lines_exact", 4: "k_ml_lines", 5: "k_ml_accum", 6: "k_ml_merge", 7: "k_ml_horner"}
        for kind, ms in kt:
            solo[names.get(kind, str(kind))] = solo.get(names.get(kind, str(kind)), 0.0) + ms
    eng.set_mp_threshold(4096)
    lat = {}
    if full and rank == 0 and not args.no_latency:
        # the throughput-against-batch curve of ONE call (the headline needs 524 800 pairs in flight per step): the literal
        # configs among them -- 1025 pairs = configs[1], 8192 = the per-GPU shard of configs[2], 65 536 = configs[2] on one GPU
        for m in (1, 2, 5, 64, 512, 1025, 2048, 4096, 8192, 16384, 65536, 262144, 1048576):
            reps = (m + len(g1) // 96 - 1) // (len(g1) // 96)
            x1, x2 = env.up((g1 * reps)[:96 * m]), env.up((g2 * reps)[:192 * m])
            eng.reserve(m)
            ms = latency_probe(env, eng, x1, x2, m, streams[0], reps=4 if m <= 65536 else 2)
            lat["%d_pairs" % m] = {"latency_ms": ms, "pairings_per_s": m / (ms * 1e-3)}
            del x1, x2

    # c3: what ONE rank of an 8-GPU node would do, timed here on one GPU with the very entries the sharded step uses -- the
    # Miller loops + product of a 8192-pair shard (blsgpu_miller_product_batch_dev), the final exponentiation of the product
    # of 8 gathered partials (blsgpu_final_exp_product_batch_dev) -- so that the first measured SCALE line can be read
    # against a stated expectation; the all-gather of 8 x 576 bytes is a latency (assumed 0.05 ms, not measured here)
    projection = None
    if full and c3 and rank == 0 and world == 1 and not args.no_latency:
        shard_pairs, ranks8 = args.pairs_total // 8, 8
        x1, x2 = env.up(g1[:96 * shard_pairs]), env.up(g2[:192 * shard_pairs])
        p8 = torch.zeros(ranks8 * 144, dtype=torch.int32, device=dev)
        o8 = torch.zeros(576, dtype=torch.uint8, device=dev)
        eng.reserve(shard_pairs + 3)
        st0 = streams[0].cuda_stream

        def timed(fn, reps=4):
            best = 1e9
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(streams[0]); fn(); e1.record(streams[0]); streams[0].synchronize()
                best = min(best, e0.elapsed_time(e1))
            return best
        t_mil = timed(lambda: eng.miller_product_batch_dev(x1.data_ptr(), x2.data_ptr(), shard_pairs, 1, p8.data_ptr(), st0))
        for r in range(1, ranks8):                       # eight copies of that partial stand in for the gathered ones
            p8[r * 144:(r + 1) * 144] = p8[:144]
        t_fin = timed(lambda: eng.final_exp_product_batch_dev(p8.data_ptr(), ranks8, 1, o8.data_ptr(), st0))
        gather_ms = 0.05
        projection = {"ranks": ranks8, "pairs_per_rank": shard_pairs, "miller_and_product_ms": t_mil, "all_gather_ms_assumed": gather_ms,
                      "final_exp_of_8_partials_ms": t_fin, "step_ms": t_mil + gather_ms + t_fin,
                      "pairings_per_s": args.pairs_total / ((t_mil + gather_ms + t_fin) * 1e-3),
                      "speedup_over_this_gpu_alone": (dt / args.steps * 1e3) / (t_mil + gather_ms + t_fin)}
        del x1, x2
    if rank == 0:
        total_pairs = sum(i["pairs"] for i in info) * args.steps
        value = total_pairs / dt
        check = "not checked (bench.py --full checks the results)"
        if full:
            tot = [sum(i["sums"][v] for i in info) % N_ORDER for v in range(B)]
            want = bilinear_expectation(eng, gen1, gen2, tot)
            check = "bilinear-ok" if per == want else "MISMATCH"
            if not c3 and n == 1025 and check != "MISMATCH" and world == 1:
                # verification 0 = the batch whose result the reference produced
                check = "golden+bilinear-ok" if per[0].hex() == gj["seeded"]["1025"]["out"] else "MISMATCH"
            elif not c3 and check != "MISMATCH":
                # verification 0 is the multi-pairing of the PRF pairs 0 .. world * n - 1 (rank r holds the slice
                # [r n, (r + 1) n)): for 8192 / 65 536 pairs in all the reference produced its value
                ref = os.path.join(gold, "pairing_seeded_%d.json" % (n * world))
                if os.path.exists(ref):
                    with open(ref) as f:
                        check = "reference-digest+bilinear-ok" if per[0].hex() == json.load(f)["out"] else "MISMATCH"
            if c3 and check != "MISMATCH":
                # the ONE multi-pairing of c3 is the reference's own for 8192 / 65 536 pairs (fixtures generated by
                # importing the reference, tests/golden/make_golden.py seeded8192 / seeded65536): whatever the sharding
                ref = os.path.join(gold, "pairing_seeded_%d.json" % args.pairs_total)
                if os.path.exists(ref):
                    with open(ref) as f:
                        check = "reference-digest+bilinear-ok" if per[0].hex() == json.load(f)["out"] else "MISMATCH"
            if len(set(per)) != B:
                check = "MISMATCH"                       # different batches must give different results
            if check == "MISMATCH":
                raise SystemExit("result mismatch -- bench invalid")
        # dominant kernel = the Miller kernel (all the per-pairing work): algorithmic MACs of one launch
        # over its average duration in the timed region (launches do not overlap each other, see step())
        ach = MAC_PER_PAIRING * n * B / (miller_avg * 1e-3) / 1e12
        if line_stream:
            kname = "k_ml_lines+k_ml_accum+k_ml_merge+k_ml_horner"
            alg_bytes = (HBM_BYTES_PER_PAIRING + 2 * LS_LINE_BYTES_PER_PAIRING) * n * B
        else:
            kname = "k_miller_mp" if n * B >= 2048 else "k_miller"
            alg_bytes = HBM_BYTES_PER_PAIRING * n * B + 576 * ((n + 2) // 3) * B
        traffic, traffic_src = pmc_traffic(kname.split("+"), n * B)
        if c3:
            workload = ("ONE multi-pairing of %d pairs sharded over %d GPU(s) (%d pairs per GPU), one final exponentiation "
                        "(BASELINE configs[2])" % (args.pairs_total, world, n))
            par = "shard%d+allgather576B" % world
        else:
            workload = ("%d independent aggregate verifications per step, each a multi-pairing of %d (pk, H(m)) pairs per GPU "
                        "with its own final exponentiation (BASELINE configs[1] shape x %d); %d different PRF-seeded pairs per GPU"
                        % (B, n, B, n * B))
            par = "shard%d+allgather%dB" % (world, 576 * B)
        line = {
            "metric": "BLS12-381 pairings/sec (aggregate_verify multi-pairing)",
            "value": value, "unit": "pairings/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True,
            "scaling": "strong" if c3 else "weak", "vs_baseline": None,
            "dtype": "i32 limbs of 28 bits, i64 accumulators" if line_stream else "u32", "data": "synthetic",
            "config": {"workload": workload, "name": args.config, "pairs_per_verification_per_gpu": n, "verifications_per_step": B,
                       "pairs_per_step_per_gpu": n * B, "parallelism": par, "steps_in_flight": S, "check": check,
                       "backend": env.backend if env.dist else "none", "ranks_in_process_group": len(info)},
            "roofline": {"bound": "valu-int32-mac", "achieved": ach, "peak": PEAK_TMACS, "unit": "TMAC/s",
                         "frac": ach / PEAK_TMACS, "traffic": traffic,
                         # the same against the multiply-add rate a 30 ms probe kernel reached in THIS run right before the timed steps
                         "peak_measured_this_run": getattr(env, "peak_now", None),
                         "frac_of_peak_measured_this_run": (ach / env.peak_now) if getattr(env, "peak_now", None) else None,
                         "traffic_unit": "bytes per launch, offline rocprofv3 --pmc FETCH_SIZE + WRITE_SIZE (%s)" % traffic_src,
                         "algorithmic_bytes_per_launch": alg_bytes,
                         "kernel": kname,
                         "kernel_launches_timed": launches, "kernel_ms_avg": miller_avg,
                         "pairings_per_launch": n * B, "mac_per_pairing": MAC_PER_PAIRING,
                         # (overlapped: these few-wavefront kernels of step i run beside the chip-filling point chains of step
                         # i + 1 and are stretched by them; *_solo_ms: the same kernels of one step alone on the idle GPU)
                         "reduce_kernels_ms_per_step_overlapped": sum(reduce_ms) / max(1, launches),
                         "degenerate_pair_kernel_ms_per_step": sum(slow_ms) / max(1, launches),
                         "final_exp_kernel_ms_avg_overlapped": (sum(fexp_ms) / len(fexp_ms)) if fexp_ms else None,
                         "one_step_alone_kernel_ms": solo,
                         # the step's working set (sampled right after the timed steps); the later probes of this run (single
                         # calls of up to 2^20 pairs, the other configs) grow context 0 further: its high-water mark beside it
                         "hbm_workspace_bytes": ws_after_steps,
                         "hbm_workspace_bytes_high_water_after_all_probes": {"context_0": eng.workspace_bytes()["total"]},
                         "whole_step_TMACs": (MAC_PER_PAIRING * n + MAC_PER_FINAL_EXP) * B * world / (dt / args.steps) / 1e12,
                         "step_latency_ms_avg": sum(step_ms) / len(step_ms), "step_latency_ms_min": step_ms[0],
                         "hbm_GBps_algorithmic": alg_bytes / (miller_avg * 1e-3) / 1e9,
                         "hbm_peak_GBps": PEAK_HBM_GBS,
                         # the engine clock / package power rank 0's GPU ran the timed steps at (sysfs samples): `peak` is the
                         # multiply-add rate measured at the power-limited clock (65 536 lanes x 2.115 GHz / 4), not at 2.4 GHz
                         "gpu_clock_during_timed_steps": getattr(env, "clock", None),
                         # the same achieved rate against the multiply-add issue rate AT THAT CLOCK (65 536 lanes, one
                         # v_mad_i64_i32 per 4 cycles): what the kernels do with the cycles the power limit leaves them
                         "frac_of_issue_rate_at_measured_clock": (ach / (65536 * env.clock["sclk_mhz_median"] * 1e6 / 4 / 1e12))
                         if getattr(env, "clock", None) else None},
            "per_rank": [{"rank": i["rank"], "device": i["device"], "k_miller_ms_avg": i["k_miller_ms_avg"]} for i in info],
            "single_call_latency": lat,
        }
        if projection:
            line["projected_8_gpu_step"] = projection
        if line_stream:
            # the stage's kernels one by one; k_ml_accum also by the multiply-accumulates it EXECUTES (round 5: three sums of
            # three products, 3 x 4 x 196 v_mad_i64_i32 per line product per lane -- 2 x 7 x 196 in rounds 3 - 4 --, six lanes;
            # 68 lines per pair) against the measured rate of that instruction (profiles/r03_fp28_microbench.txt: 34.1 T/s at
            # four wavefronts per SIMD)
            exec_mads = 3 * 4 * 196 * 6 * LS_LINES * n * B
            line["roofline"]["stage_kernels_ms_avg"] = ls_avg
            line["roofline"]["k_ml_accum_executed_mad28_Tps"] = exec_mads / (ls_avg["k_ml_accum"] * 1e-3) / 1e12
            line["roofline"]["k_ml_accum_frac_of_mad_i64_i32_peak"] = exec_mads / (ls_avg["k_ml_accum"] * 1e-3) / 1e12 / PEAK_MAD28_T
            # the point-chain kernel likewise: v_mad_i64_i32 per wavefront and step read off the ISA of the shipped build
            # (tangent step 4718 -- 5320 before the mixed products became squares in round 4 --, chord step 8847; 32 pairs per
            # wavefront, both lanes of a pair count)
            lines_mads = (63 * 4718 + 5 * 8847) * 2 * n * B
            line["roofline"]["k_ml_lines_executed_mad28_Tps"] = lines_mads / (ls_avg["k_ml_lines"] * 1e-3) / 1e12
            line["roofline"]["k_ml_lines_frac_of_mad_i64_i32_peak"] = lines_mads / (ls_avg["k_ml_lines"] * 1e-3) / 1e12 / PEAK_MAD28_T
            line["roofline"]["executed_mad28_per_pairing"] = (exec_mads + lines_mads) / (n * B)
            line["roofline"]["stage_frac_by_executed_work"] = (exec_mads + lines_mads) / (miller_avg * 1e-3) / 1e12 / PEAK_MAD28_T
            line["roofline"]["note"] = ("frac credits SURVEY 8(d)'s 2.026 M MAC32 per pairing, which counts a 36 m squaring of the accumulator "
                                        "per pair and step (this design squares once per GROUP in the Horner kernel) and 300 MAC32 per Fq "
                                        "product (28-bit limbs execute 392); the two nearly cancel: executed_mad28_per_pairing / "
                                        "stage_frac_by_executed_work state what the two kernels really issue")
        if full and not args.no_cpu_baseline and world == 1:
            cb = cpu_baseline(g1[:96 * min(n, 1025)], g2[:192 * min(n, 1025)], min(n, 1025), per[0] if n == 1025 else None)
            if not cb["matches_gpu"]:
                raise SystemExit("CPU oracle and GPU disagree -- bench invalid")
            line["cpu_baseline"] = cb
        if full and not c3 and world == 1 and not args.no_secondary:
            line["secondary"] = secondary(env, args, eng, gen1, gen2)
        return line
    return None


def secondary(env, args, eng, gen1, gen2):
    """The other BASELINE configs once each, after the timed region (N = 1 only): c3 = ONE 65 536-pair multi-pairing
    against the reference's digest, c4, c5, h2c as `--config` runs them (2 timed repetitions).  Every entry carries the
    check it passed; a mismatch aborts the bench like the headline's."""
    torch = env.torch
    out = {}
    # c3: the 65 536 pairs of tests/golden/pairing_seeded_65536.json (PRF indices 0 .. 65535), one call, one final exponentiation
    n3 = C3_PAIRS
    g1, g2, _, _ = seeded_points(eng, gen1, gen2, list(range(n3)))
    x1, x2 = env.up(g1), env.up(g2)
    o3 = torch.zeros(576, dtype=torch.uint8, device=env.dev)
    eng.reserve(n3 + 3)
    eng.set_mp_threshold(4096)
    st = torch.cuda.current_stream().cuda_stream
    dt3 = device_timed(env, lambda: eng.pairing_multi_dev(x1.data_ptr(), x2.data_ptr(), n3, o3.data_ptr(), st), 3)
    with open(os.path.join(ROOT, "tests", "golden", "pairing_seeded_%d.json" % n3)) as f:
        if bytes(o3.cpu().numpy()).hex() != json.load(f)["out"]:
            raise SystemExit("c3 result differs from the reference's digest -- bench invalid")
    out["c3"] = {"value": n3 / dt3, "unit": "pairings/s", "ms": dt3 * 1e3, "check": "reference-digest-ok",
                 "workload": "ONE multi-pairing of %d pairs on one GPU incl. its final exponentiation (BASELINE configs[2] unsharded)" % n3,
                 "roofline_frac": (MAC_PER_PAIRING * n3 + MAC_PER_FINAL_EXP) / dt3 / 1e12 / PEAK_TMACS}
    del x1, x2
    sub = argparse.Namespace(**vars(args))
    sub.steps = 2
    for name, fn in (("c4", run_c4), ("c5", run_c5), ("h2c", run_h2c)):
        ln = fn(env, sub)
        out[name] = {"value": ln["value"], "unit": ln["unit"], "ms": ln["ms_per_step"], "check": ln["config"]["check"],
                     "workload": ln["config"]["workload"], "roofline_frac": ln["roofline"]["frac"],
                     "traffic": ln["roofline"].get("traffic"), "traffic_source": ln["roofline"].get("traffic_source"),
                     "algorithmic_bytes": ln["roofline"].get("algorithmic_bytes")}
        if name == "c4":
            out[name].update(combine_ms=ln["combine_s"] * 1e3, verify_ms=ln["verify_s"] * 1e3)
    out["verify_pipeline"] = run_verify_pipeline(env, eng)
    out["verify_single_signature"] = run_verify_single(env, eng)
    out["g2_sum"] = run_g2_sum(env, eng, gen2)
    out["other_shapes"] = run_other_shapes(env, eng, gen1, gen2)
    return out


def run_other_shapes(env, eng, gen1, gen2, n=65536):
    """The entry points in the call shapes BASELINE.json does not name (tools/shape_sweep.py): a batch of scalar
    multiplications (groups x 1 point: key generation, signing), ONE plain sum of the results (aggregate_pub_keys / aggregate_sigs
    without exponents), and the reference's own fq_miller_loop value per pair (blsgpu_miller_loop_batch).  Device-resident, each
    with a check that does not go through the kernel it checks."""
    torch = env.torch
    from bls_py import _native
    old = {k: os.environ.get(k) for k in ("BLSGPU_MSM_SORT_THRESHOLD", "BLSGPU_MSM_SORT2_THRESHOLD", "BLSGPU_MSM_PLAIN_THRESHOLD", "BLSGPU_SMUL_MIN_GROUPS")}
    for k in old:
        os.environ[k] = str(1 << 40)
    try:
        vm = _native.Engine(env.local_dev)                       # the wavefront VM's / fixed-window kernels: the independent side of the checks
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    a = [prf_scalar(b"blsgpu/shapes/a", 0, i) for i in range(n)]
    sc = env.up(b"".join(x.to_bytes(32, "big") for x in a))
    st = torch.cuda.current_stream().cuda_stream
    res = {}
    pts = {}
    for deg, gen, fn in ((1, gen1, "blsgpu_g1_msm_dev"), (2, gen2, "blsgpu_g2_msm_dev")):
        sz = 96 * deg
        dp, do, fl = env.up(gen * n), torch.zeros(sz * n, dtype=torch.uint8, device=env.dev), torch.zeros(n, dtype=torch.uint8, device=env.dev)
        f = getattr(eng.lib, fn)
        dt = device_timed(env, lambda: f(eng.h, dp.data_ptr(), sc.data_ptr(), 1, n, do.data_ptr(), fl.data_ptr(), st), 2)
        got = bytes(do.cpu().numpy())
        probe = [0, 1, n // 2, n - 1]
        want = (vm.g1_msm if deg == 1 else vm.g2_msm)(gen * len(probe), [a[i] for i in probe], 1, len(probe))[0]
        if b"".join(got[sz * i:sz * (i + 1)] for i in probe) != want:
            raise SystemExit("other_shapes: a scalar multiplication of the batch differs from the fixed-window kernels' -- bench invalid")
        res["scalar_multiplications_g%d" % deg] = {"value": n / dt, "unit": "points/s", "ms": dt * 1e3, "batch": n}
        pts[deg] = do
        # one plain sum of the n results: sum a_i G == (sum a_i) G
        out1, inf1 = torch.zeros(sz, dtype=torch.uint8, device=env.dev), torch.zeros(1, dtype=torch.uint8, device=env.dev)
        dt = device_timed(env, lambda: f(eng.h, do.data_ptr(), None, n, 1, out1.data_ptr(), inf1.data_ptr(), st), 3)
        want = (vm.g1_msm if deg == 1 else vm.g2_msm)(gen, [sum(a) % N_ORDER], 1, 1)[0]
        if bytes(out1.cpu().numpy()) != want:
            raise SystemExit("other_shapes: sum a_i G != (sum a_i) G -- bench invalid")
        res["plain_sum_g%d" % deg] = {"value": n / dt, "unit": "points/s", "ms": dt * 1e3, "points": n}
    # the reference's Miller value of every pair (a_i G1, a_i G2); check: its final exponentiation is the pairing of the pair
    om = torch.zeros(576 * n, dtype=torch.uint8, device=env.dev)
    dt = device_timed(env, lambda: eng.miller_loop_batch_dev(pts[1].data_ptr(), pts[2].data_ptr(), n, om.data_ptr(), st), 2)
    dt1 = device_timed(env, lambda: eng.miller_loop_batch_dev(pts[1].data_ptr(), pts[2].data_ptr(), 1, om.data_ptr(), st), 3)
    eng.miller_loop_batch_dev(pts[1].data_ptr(), pts[2].data_ptr(), n, om.data_ptr(), st)
    torch.cuda.synchronize()
    g1b, g2b, mb = bytes(pts[1][:96 * 3].cpu().numpy()), bytes(pts[2][:192 * 3].cpu().numpy()), bytes(om[:576 * 3].cpu().numpy())
    for i in range(3):
        if eng.final_exp(mb[576 * i:576 * (i + 1)]) != eng.pairing_multi(g1b[96 * i:96 * (i + 1)], g2b[192 * i:192 * (i + 1)], 1):
            raise SystemExit("other_shapes: final_exp(miller_loop_batch value) != pairing -- bench invalid")
    res["miller_loop_batch"] = {"value": n / dt, "unit": "pairs/s", "ms": dt * 1e3, "pairs": n, "one_pair_ms": dt1 * 1e3}
    res["check"] = ("scalar multiplications: four of the batch against the fixed-window kernels; plain sums: sum a_i G == (sum a_i) G from those "
                    "kernels; Miller values: their final exponentiation == the pairing of the pair (tests/test_gpu_parity.py holds them to the "
                    "reference's golden fq_miller_loop values)")
    return res


def run_g2_sum(env, eng, gen2, n=16384):
    """ONE G2 sum with scalars -- BLS.aggregate_sigs(secure) (bls.py:225-261) as a multi-scalar sum, SURVEY 8(f) rank 2 -- on
    device-resident buffers: n different points a_i G2 with PRF scalars t_i through the default selection (sorted buckets on lane
    pairs), checked by  sum t_i (a_i G2) == (sum t_i a_i) G2  with the right-hand side from an engine WITHOUT the
    sorted buckets (the fixed-window kernels), which is also timed on the same input."""
    torch = env.torch
    from bls_py import _native
    a = [prf_scalar(b"blsgpu/g2sum/a", 0, i) for i in range(n)]
    t = [prf_scalar(b"blsgpu/g2sum/t", 0, i) for i in range(n)]
    pts, _ = eng.g2_msm(gen2 * n, a, 1, n)
    old = {k: os.environ.get(k) for k in ("BLSGPU_MSM_SORT2_THRESHOLD",)}
    os.environ["BLSGPU_MSM_SORT2_THRESHOLD"] = str(1 << 40)
    try:
        fixed = _native.Engine(env.local_dev)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    want, _ = fixed.g2_msm(gen2, [sum(x * y for x, y in zip(a, t)) % N_ORDER], 1, 1)
    dp, ds = env.up(pts), env.up(b"".join(x.to_bytes(32, "big") for x in t))
    out = torch.zeros(192, dtype=torch.uint8, device=env.dev)
    inf = torch.zeros(1, dtype=torch.uint8, device=env.dev)
    st = torch.cuda.current_stream().cuda_stream
    res = {}
    for name, e in (("sorted", eng), ("fixed_windows", fixed)):
        out.zero_()
        dt = device_timed(env, lambda: e.lib.blsgpu_g2_msm_dev(e.h, dp.data_ptr(), ds.data_ptr(), n, 1, out.data_ptr(), inf.data_ptr(), st), 3)
        if bytes(out.cpu().numpy()) != want:
            raise SystemExit("g2_sum (%s): sum t_i (a_i G2) != (sum t_i a_i) G2 -- bench invalid" % name)
        res[name] = dt
    return {"value": n / res["sorted"], "unit": "points/s", "ms": res["sorted"] * 1e3, "fixed_window_kernels_ms": res["fixed_windows"] * 1e3,
            "check": "sum t_i (a_i G2) == (sum t_i a_i) G2, right-hand side from the fixed-window kernels; both paths give it",
            "workload": "ONE G2 multi-scalar sum of %d points with 256-bit scalars (aggregate_sigs(secure) as a multi-scalar sum): sorted buckets, "
                        "13-bit windows of signed digits, a piece of the sorted list per lane pair, the tail one wavefront per chain" % n}


def run_verify_single(env, eng):
    """BLS.verify of ONE signature (bls.py:153-201): hash the one message hash to G2 (ec.py:528-550), then the two-pair
    multi-pairing e(-G1, sig) e(pk, H(m)) and its final exponentiation -- blsgpu_verify_pipeline_dev on device-resident
    buffers, and the host-buffer entry (one upload, 576 bytes back: PCIe and the host's launch path included).  Latency, not
    throughput: the call is a chain of a few wavefronts (csrc/blsgpu_mlw.hip, blsgpu_fexpw.hip)."""
    torch = env.torch
    from bls_py import hostmath as H
    from bls_py.keys import PrivateKey
    sk = PrivateKey(int.from_bytes(hashlib.sha256(b"single").digest(), "big") % (N_ORDER - 1) + 1)
    msg = b"one message"
    sig = sk.sign(msg)
    mh = hashlib.sha256(msg).digest()
    pk = H.g1_affine_bytes(sig.aggregation_info.public_keys[0].value.to_affine()._aff())
    neg_g1 = H.g1_affine_bytes(H.jac_to_affine(H.F1, H.jac_mul(H.F1, H.aff_to_jac(H.F1, H.G1_GEN), N_ORDER - 1)))
    sig_b = H.g2_affine_bytes(sig.value.to_affine()._aff())
    d_g1 = env.up(neg_g1 + pk)
    d_g2 = env.up(sig_b + bytes(192))
    d_mh = env.up(mh)
    d_h = torch.zeros(192, dtype=torch.uint8, device=env.dev)
    d_out = torch.zeros(576, dtype=torch.uint8, device=env.dev)
    stream = torch.cuda.Stream(device=env.dev)
    st = stream.cuda_stream
    lib, h = eng.lib, eng.h

    def timed(fn, reps=6):
        fn(); stream.synchronize()
        best = 1e9
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream); fn(); b.record(stream); stream.synchronize()
            best = min(best, a.elapsed_time(b))
        return best
    ms_all = timed(lambda: lib.blsgpu_verify_pipeline_dev(h, d_g1.data_ptr(), d_g2.data_ptr(), d_mh.data_ptr(), 1, None, None, 0, d_out.data_ptr(), st))
    one = (1).to_bytes(48, "big") + bytes(48 * 11)
    if bytes(d_out.cpu().numpy()) != one:
        raise SystemExit("verify_single_signature: the signature did not verify -- bench invalid")
    ms_hash = timed(lambda: lib.blsgpu_hash_to_g2_dev(h, d_mh.data_ptr(), 1, d_h.data_ptr(), st))
    ms_pair = timed(lambda: eng.pairing_multi_dev(d_g1.data_ptr(), d_g2.data_ptr(), 2, d_out.data_ptr(), st))
    t = time.perf_counter()
    reps = 20
    for _ in range(reps):
        got = eng.verify_pipeline(neg_g1, sig_b, mh, 1, keys_affine=pk)
    wall = (time.perf_counter() - t) / reps
    if got != one:
        raise SystemExit("verify_single_signature (host buffers): the signature did not verify -- bench invalid")
    # a tampered message must NOT verify
    bad = eng.verify_pipeline(neg_g1, sig_b, hashlib.sha256(b"another message").digest(), 1, keys_affine=pk)
    if bad == one:
        raise SystemExit("verify_single_signature: a wrong message verified -- bench invalid")
    return {"value": ms_all, "unit": "ms", "higher_is_better": False, "check": "result == Fq12 one; a different message does not verify",
            "workload": "BLS.verify of one signature on device-resident buffers: hash one message to G2 + two-pair multi-pairing + final exponentiation (blsgpu_verify_pipeline_dev)",
            "hash_to_g2_of_one_message_ms": ms_hash, "two_pair_multi_pairing_ms": ms_pair,
            "host_buffer_entry_wall_ms": wall * 1e3}


def run_verify_pipeline(env, eng, B=256, n=1024):
    """The device part of B x BLS.verify (bls.py:153-201) on aggregates of n signatures over n distinct messages, everything
    resident in HBM: hash the B x n message hashes to G2 (ec.py:528-550), place them behind each aggregate signature, one
    batched (n + 1)-pair multi-pairing per aggregate, compare with one.  One key per message with exponent 1 (plain
    aggregation, bls.py:177-192).  ONE real aggregate (signed and aggregated through the package) verified B times with
    rotated message order."""
    torch = env.torch
    from bls_py import hostmath as H
    from bls_py.bls import BLS
    from bls_py.keys import PrivateKey
    sks = [PrivateKey(int.from_bytes(hashlib.sha256(b"pipe%d" % i).digest(), "big") % (N_ORDER - 1) + 1) for i in range(n)]
    msgs = [i.to_bytes(4, "big") for i in range(n)]
    sigs = PrivateKey.sign_batch(sks, msgs)
    agg = BLS.aggregate_sigs(sigs)
    mh = [hashlib.sha256(m).digest() for m in msgs]
    pks = [H.g1_affine_bytes(s.aggregation_info.public_keys[0].value.to_affine()._aff()) for s in sigs]
    neg_g1 = H.g1_affine_bytes(H.jac_to_affine(H.F1, H.jac_mul(H.F1, H.aff_to_jac(H.F1, H.G1_GEN), N_ORDER - 1)))
    sig_b = H.g2_affine_bytes(agg.value.to_affine()._aff())
    g1_all, mh_all = bytearray(), bytearray()
    for v in range(B):
        order = [(i + 31 * v) % n for i in range(n)]
        g1_all += neg_g1 + b"".join(pks[i] for i in order)
        mh_all += b"".join(mh[i] for i in order)
    d_g1, d_mh = env.up(g1_all), env.up(mh_all)
    d_g2 = torch.zeros(B * (n + 1) * 192, dtype=torch.uint8, device=env.dev).view(B, n + 1, 192)
    d_g2[:, 0, :] = env.up(sig_b)
    d_h = torch.zeros(B * n * 192, dtype=torch.uint8, device=env.dev)
    d_out = torch.zeros(B * 576, dtype=torch.uint8, device=env.dev)
    eng.reserve((n + 4) * B)
    eng.set_mp_threshold(0)
    st = torch.cuda.current_stream().cuda_stream

    def run():
        eng.lib.blsgpu_hash_to_g2_dev(eng.h, d_mh.data_ptr(), B * n, d_h.data_ptr(), st)
        d_g2[:, 1:, :] = d_h.view(B, n, 192)
        eng.pairing_multi_batch_dev(d_g1.data_ptr(), d_g2.data_ptr(), n + 1, B, d_out.data_ptr(), st)
    dt = device_timed(env, run, 3)
    one = (1).to_bytes(48, "big") + bytes(48 * 11)
    if bytes(d_out.cpu().numpy()) != one * B:
        raise SystemExit("verify pipeline: an aggregate did not verify -- bench invalid")
    eng.set_mp_threshold(4096)
    return {"value": B * n / dt, "unit": "signatures/s", "ms": dt * 1e3, "check": "every aggregate verifies (result == Fq12 one)",
            "workload": "%d aggregate verifications x %d messages, device resident: hash to G2 + %d-pair multi-pairing each" % (B, n, n + 1)}


def device_timed(env, fn, reps, mark=None):
    """seconds per call of fn over `reps` back-to-back calls (HIP events); mark: an engine whose empty marker kernel brackets
    the calls in a profile of the run"""
    torch = env.torch
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if mark is not None:
        mark.mark(1)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    if mark is not None:
        mark.mark(2)
    return a.elapsed_time(b) * 1e-3 / reps


def run_c4(env, args):
    """C4: 10 000 groups x (67-point G2 multi-scalar combine + two-pair verify).  Groups shard over
    ranks with no exchange (weak scaling: 10 000 groups per GPU)."""
    torch = env.torch
    from bls_py import _native, hostmath as H, util
    from bls_py.keys import PublicKey
    eng = _native.Engine(env.local_dev)
    with open(os.path.join(ROOT, "tests", "golden", "threshold.json")) as f:
        th = json.load(f)["67_of_100"]
    groups, k = args.groups, 67
    pts = b"".join(bytes.fromhex(s) for s in th["unit_sigs_affine"])
    lam = [int(x, 16) for x in th["lambdas"]]
    # every group gets its own shares: group g's points are the golden shares scaled by c_g (a G2
    # group sum per share would cost more than the measurement; instead the SCALARS differ:
    # lambda_j * c_g, so that the combine of group g must equal c_g * golden)
    cg = [prf_scalar(b"blsgpu/c4", 1, env.rank * groups + g) for g in range(groups)]
    sc = b"".join(((l * c) % N_ORDER).to_bytes(32, "big") for c in cg for l in lam)
    tp, ts = env.up(pts * groups), env.up(sc)
    tout = torch.zeros(groups * 192, dtype=torch.uint8, device=env.dev)
    tinf = torch.zeros(groups, dtype=torch.uint8, device=env.dev)
    lib, h = eng.lib, eng.h
    reps = max(1, args.steps)
    dt_c = device_timed(env, lambda: lib.blsgpu_g2_msm_dev(h, tp.data_ptr(), ts.data_ptr(), k, groups, tout.data_ptr(), tinf.data_ptr(), 0), reps)
    got = bytes(tout.cpu().numpy())
    gold_pt = bytes.fromhex(th["combined_affine"])
    want, _ = eng.g2_msm(gold_pt * groups, cg, 1, groups)
    ok_c = got == want and not bool(tinf.any())
    # verify: e(-G1, sig_g) e(c_g pk, H(m)) = 1 per group
    pk = PublicKey.from_bytes(bytes.fromhex(th["master_pk"])).value.to_affine()._aff()
    hm = H.g2_affine_bytes(H.hash_to_g2_prehashed(util.hash256(bytes.fromhex(th["msg"])), util.hash512))
    ng1 = H.g1_affine_bytes(H.jac_to_affine(H.F1, H.jac_mul(H.F1, H.aff_to_jac(H.F1, H.G1_GEN), N_ORDER - 1)))
    pks, _ = eng.g1_msm(H.g1_affine_bytes(pk) * groups, cg, 1, groups)
    pg1 = b"".join(ng1 + pks[96 * g:96 * (g + 1)] for g in range(groups))
    pg2 = b"".join(got[192 * g:192 * (g + 1)] + hm for g in range(groups))
    v1, v2 = env.up(pg1), env.up(pg2)
    vout = torch.zeros(groups * 576, dtype=torch.uint8, device=env.dev)
    dt_v = device_timed(env, lambda: eng.pairing_multi_batch_dev(v1.data_ptr(), v2.data_ptr(), 2, groups, vout.data_ptr(), 0), reps)
    one = (1).to_bytes(48, "big") + bytes(48 * 11)
    ok_v = bytes(vout.cpu().numpy()) == one * groups
    # The timed step: combine -> the combined signatures into the verifies' G2 operands (on the device) -> verify, with
    # --streams steps in flight on contexts of their own (the Horner / small-group Miller / final-exponentiation kernels
    # of 10 000 groups leave SIMDs empty; the next step's bucket sums fill them).  combine_s / verify_s above: each alone.
    S = max(1, args.streams)
    engs = [eng] + [_native.Engine(env.local_dev) for _ in range(S - 1)]
    streams = [torch.cuda.Stream(device=env.dev) for _ in range(S)]
    touts = [torch.zeros(groups * 192, dtype=torch.uint8, device=env.dev) for _ in range(S)]
    tinfs = [torch.zeros(groups, dtype=torch.uint8, device=env.dev) for _ in range(S)]
    v2s = [v2.clone() for _ in range(S)]
    vouts = [torch.zeros(groups * 576, dtype=torch.uint8, device=env.dev) for _ in range(S)]
    for j in range(S):
        v2s[j].view(groups, 2, 192)[:, 0, :].zero_()

    def step(i):
        j = i % S
        e, st = engs[j], streams[j]
        e._check(e.lib.blsgpu_g2_msm_dev(e.h, tp.data_ptr(), ts.data_ptr(), k, groups, touts[j].data_ptr(), tinfs[j].data_ptr(), st.cuda_stream), "g2_msm_dev")
        with torch.cuda.stream(st):
            v2s[j].view(groups, 2, 192)[:, 0, :].copy_(touts[j].view(groups, 192))
        e.pairing_multi_batch_dev(v1.data_ptr(), v2s[j].data_ptr(), 2, groups, vouts[j].data_ptr(), st.cuda_stream)
    for i in range(S):
        step(i)
    torch.cuda.synchronize()
    env.barrier()
    eng.mark(1)
    t0 = time.perf_counter()
    for i in range(reps):
        step(i)
    torch.cuda.synchronize()
    env.barrier()
    dt_step = (time.perf_counter() - t0) / reps
    eng.mark(2)
    ok_p = all(bytes(vo.cpu().numpy()) == one * groups for vo in vouts) and all(bytes(t.cpu().numpy()) == want for t in touts)
    dt = env.max_over_ranks(dt_step)
    oks = env.gather_objects(ok_c and ok_v and ok_p)
    if env.rank == 0:
        if not all(oks):
            raise SystemExit("result mismatch -- bench invalid")
        # algorithmic work: bucket method, 4-bit windows: 64 windows x (67 + 2 x 15) mixed G2
        # additions of 36 Fq-mults; two Miller loops + one final exponentiation per verify
        mac_combine = 64 * (k + 30) * 36 * MAC_PER_FQ_MUL
        mac_verify = 2 * MAC_PER_PAIRING + MAC_PER_FINAL_EXP
        return {
            "metric": "threshold groups/sec (k=67 of n=100: combine + verify)", "value": groups * env.world / dt, "unit": "groups/s",
            "n_gpus": env.world, "steps": reps, "warmup": 1, "ms_per_step": dt * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "u32", "data": "synthetic",
            "config": {"workload": "BASELINE configs[3]: %d groups per GPU, G2 multi-scalar combine of 67 shares + 2-pair verify; "
                                   "bucket method with signed 4-bit digits, one (group, window) per lane PAIR (Fq2 split over two lanes), 8 buckets in HBM, complete mixed additions; verifies: point chains on lane pairs + one accumulator per group (k_ml_lines2, k_ml_small)" % groups, "name": "c4",
                       "steps_in_flight": S, "check": "combine == c_g x reference golden, every verify == 1 (alone and in the timed steps)"},
            "combine_s": dt_c, "verify_s": dt_v, "one_step_alone_ms": (dt_c + dt_v) * 1e3, "value_alone": groups * env.world / (dt_c + dt_v),
            "roofline": {"bound": "valu-int32-mac", "kernel": "k_msm_lane2x (+ k_lane_prep, windows, horner)", "peak": PEAK_TMACS, "unit": "TMAC/s",
                         "achieved": mac_combine * groups / dt_c / 1e12, "frac": mac_combine * groups / dt_c / 1e12 / PEAK_TMACS,
                         "verify_achieved": mac_verify * groups / dt_v / 1e12, "traffic": config_traffic("c4")[0], "traffic_source": config_traffic("c4")[1],
                         "whole_step_TMACs": (mac_combine + mac_verify) * groups / dt / 1e12,
                         "whole_step_frac": (mac_combine + mac_verify) * groups / dt / 1e12 / PEAK_TMACS,
                         "algorithmic_bytes": groups * k * (192 + 32)}}
    return None


def run_c5(env, args):
    """C5: ONE G1 multi-scalar sum over 2^20 DIFFERENT points (aggregate_pub_keys at scale), split over the ranks
    (bls_py.dist: contiguous point split, one all-gather of a 100-byte record per rank, `world` additions on every rank)."""
    torch = env.torch
    from bls_py import _native
    from bls_py.dist import GpuShardBackend, shard_bounds
    eng = _native.Engine(env.local_dev)
    shard = GpuShardBackend(eng, env.dev)
    with open(os.path.join(ROOT, "tests", "golden", "pairing.json")) as f:
        gen1 = bytes.fromhex(json.load(f)["gen"]["g1"])
    total = args.points
    lo, hi = shard_bounds(total, env.rank, env.world)
    n = hi - lo
    a = [prf_scalar(b"blsgpu/a", 5, lo + i) for i in range(n)]
    t = [prf_scalar(b"blsgpu/t", 5, lo + i) for i in range(n)]
    pts = b""
    for s0 in range(0, n, 1 << 18):                     # the points a_i G1, in slices
        m = min(1 << 18, n - s0)
        p, _ = eng.g1_msm(gen1 * m, a[s0:s0 + m], 1, m)
        pts += p
    assert len(set(pts[96 * i:96 * (i + 1)] for i in range(0, n, max(1, n // 4096)))) == len(range(0, n, max(1, n // 4096)))
    tp, ts = env.up(pts), env.up(b"".join(x.to_bytes(32, "big") for x in t))
    rec = torch.zeros(100, dtype=torch.uint8, device=env.dev)
    gath = torch.zeros(100 * env.world, dtype=torch.uint8, device=env.dev)
    tout = torch.zeros(96, dtype=torch.uint8, device=env.dev)
    tinf = torch.zeros(4, dtype=torch.uint8, device=env.dev)
    reps = max(1, args.steps)

    def one():
        if env.dist is None:
            shard._msm_dev(1, tp, ts, n, 1, tout, tinf)
            return
        shard.msm_partial_dev(1, tp, ts, n, rec)
        if env.backend == "nccl":
            shard.all_gather_into(gath, rec)
        else:
            host = [torch.zeros(100, dtype=torch.uint8) for _ in range(env.world)]
            env.dist.all_gather(host, rec.cpu())
            gath.copy_(torch.cat(host).to(env.dev))
        shard.msm_finish_dev(1, gath, env.world, tout, tinf)
    one()
    torch.cuda.synchronize()
    env.barrier()
    t0 = time.perf_counter()
    for _ in range(reps):
        one()
    torch.cuda.synchronize()
    env.barrier()
    dt_alone = (time.perf_counter() - t0) / reps
    # the timed steps: three (or --streams) sums in flight on contexts of their own (one GPU: the bit sums / Horner of one sum, a few
    # hundred wavefronts, run beside the next sum's list additions); with a process group the steps stay one after another
    # (a sum's tail is a third of its length: three in flight keep the chip busy; an explicit --streams is honoured, 1 = one after another)
    S = (args.streams if args.streams_given else 3) if env.dist is None else 1
    dt_step, ok_p = dt_alone, True
    if S > 1:
        shards = [shard] + [GpuShardBackend(_native.Engine(env.local_dev), env.dev) for _ in range(S - 1)]
        streams = [torch.cuda.Stream(device=env.dev) for _ in range(S)]
        outs = [torch.zeros(96, dtype=torch.uint8, device=env.dev) for _ in range(S)]
        infs = [torch.zeros(4, dtype=torch.uint8, device=env.dev) for _ in range(S)]

        def step(i):
            with torch.cuda.stream(streams[i % S]):
                shards[i % S]._msm_dev(1, tp, ts, n, 1, outs[i % S], infs[i % S])
        for i in range(S):
            step(i)
        torch.cuda.synchronize()
        eng.mark(1)
        t0 = time.perf_counter()
        for i in range(reps):
            step(i)
        torch.cuda.synchronize()
        dt_step = (time.perf_counter() - t0) / reps
        eng.mark(2)
        ok_p = all(bytes(o.cpu().numpy()) == bytes(tout.cpu().numpy()) for o in outs)
    dtm = env.max_over_ranks(dt_step)
    dt_alone_max = env.max_over_ranks(dt_alone)
    got = bytes(tout.cpu().numpy())
    parts = env.gather_objects(sum(x * y for x, y in zip(a, t)) % N_ORDER)       # sum t_i (a_i G) = (sum t_i a_i) G
    want, _ = eng.g1_msm(gen1, [sum(parts) % N_ORDER], 1, 1)
    check = "sum t_i (a_i G) == (sum t_i a_i) G"
    ok_ref = True
    ref = os.path.join(ROOT, "tests", "golden", "msm_seeded_%d.json" % total)
    if env.rank == 0 and os.path.exists(ref):
        # the REFERENCE's own sum over these very points and scalars (2^21 scalar multiplications of pure Python,
        # tests/golden/make_golden.py msm_seeded), and a sample of the input points as the reference computes them
        with open(ref) as f:
            fx = json.load(f)
        ok_ref = got.hex() == fx["sum_affine"] and all(pts[96 * (int(i) - lo):96 * (int(i) - lo + 1)].hex() == p for i, p in fx["sample_points"].items() if lo <= int(i) < hi)
        check = "the reference's sum over the same 2^20 points and scalars (tests/golden/msm_seeded_%d.json) + %s" % (total, check)
    oks = env.gather_objects(got == want and ok_p and ok_ref)
    if env.rank == 0:
        if not all(oks):
            raise SystemExit("result mismatch -- bench invalid")
        # algorithmic work, SURVEY 8(d): Pippenger with 16-bit windows = 16 windows x (n + 2^16) mixed G1 additions of 11
        # Fq-mults (1.9e8 Fq-mults for 2^20 points).  Executed: 20 windows of 13 bits -- 20 n list additions of 11 Fq-mults
        # plus 20 x 13 x 4096 + 20 x 8191 full additions (12) for the buckets' bit sums and continuation pieces.
        mac = 16 * (total + 65536) * 11 * MAC_PER_FQ_MUL
        executed = (20 * total * 11 + (20 * 13 * 4096 + 20 * 8191) * 12) * MAC_PER_FQ_MUL
        return {
            "metric": "G1 multi-scalar-sum points/sec", "value": total / dtm, "unit": "points/s", "n_gpus": env.world,
            "steps": reps, "warmup": 1, "ms_per_step": dtm * 1e3, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": "u32", "data": "synthetic",
            "config": {"workload": "BASELINE configs[4]: ONE G1 multi-scalar sum over %d different PRF points, %d per GPU; sorted buckets: "
                                   "13-bit windows of signed digits, counting sort of the (window, |digit|) keys, equal pieces of the sorted list per lane "
                                   "(complete mixed additions on 28-bit limbs in registers), bit sums of the buckets, folds / window sums / Horner "
                                   "on one wavefront per chain with a product per lane (DESIGN.md 2d)" % (total, n),
                       "name": "c5", "parallelism": "points split %d ways + all-gather of 100 B per rank" % env.world,
                       "steps_in_flight": S, "check": check},
            "one_step_alone_ms": dt_alone * 1e3, "value_alone": total / dt_alone_max,
            "roofline": {"bound": "valu-int32-mac", "kernel": "k_srt_accum (+ k_srt_prep, k_srt_count/scan/scatter/fix/bits, k_msm_lane_fold, k_msm_horner_wide)",
                         "peak": PEAK_TMACS, "unit": "TMAC/s", "achieved": mac / dtm / 1e12 / env.world, "frac": mac / dtm / 1e12 / PEAK_TMACS / env.world,
                         "traffic": config_traffic("c5")[0], "traffic_source": config_traffic("c5")[1],
                         "executed_TMACs": executed / dtm / 1e12 if total == 1 << 20 and env.world == 1 else None,
                         "algorithmic_bytes": total * (96 + 32), "hbm_GBps_algorithmic": total * 128 / dtm / 1e9}}
    return None


def run_h2c(env, args):
    torch = env.torch
    from bls_py import _native, hostmath as H, util
    eng = _native.Engine(env.local_dev)
    n = args.messages
    msgs = b"".join(hashlib.sha256(b"bench-h2c-%d-%d" % (env.rank, i)).digest() for i in range(n))
    tin = env.up(msgs)
    tout = torch.zeros(n * 192, dtype=torch.uint8, device=env.dev)
    reps = max(1, args.steps)
    dt = device_timed(env, lambda: eng.lib.blsgpu_hash_to_g2_dev(eng.h, tin.data_ptr(), n, tout.data_ptr(), 0), reps, mark=eng)
    got = bytes(tout.cpu().numpy())
    # check: the REFERENCE's digest of these very outputs where a committed fixture holds it (rank 0's first 16 384 / 20 000
    # messages: tests/golden/h2c_20000.json, produced by importing the reference), else three messages against the host
    # integer code (tests/test_hostmath_fixtures.py pins that to 1024 + 20 reference hashes)
    check = None
    if env.rank == 0 and n in (16384, 20000):
        with open(os.path.join(ROOT, "tests", "golden", "h2c_20000.json")) as f:
            fx = json.load(f)
        ok = hashlib.sha256(got).hexdigest() == fx["outputs_sha256_first_16384" if n == 16384 else "outputs_sha256"]
        check = "sha256 of all %d outputs == the reference's (tests/golden/h2c_20000.json)" % n
    else:
        ok = all(got[192 * i:192 * (i + 1)] == H.g2_affine_bytes(H.hash_to_g2_prehashed(msgs[32 * i:32 * (i + 1)], util.hash512))
                 for i in (0, n // 2, n - 1)) and len(set(got[192 * i:192 * (i + 1)] for i in range(0, n, max(1, n // 512)))) > 1
    dtm = env.max_over_ranks(dt)
    oks = env.gather_objects(ok)
    if env.rank == 0:
        if not all(oks):
            raise SystemExit("result mismatch -- bench invalid")
        # algorithmic work per message: 2 encodings x 5 fixed powers of ~380 squarings + 64 projective G2 steps of cofactor clearing
        mac = (2 * 5 * 380 * 2 + 2 * 64 * 36 + 400) * MAC_PER_FQ_MUL
        return {
            "metric": "hash-to-G2 messages/sec", "value": n * env.world / dtm, "unit": "messages/s", "n_gpus": env.world, "steps": reps,
            "warmup": 1, "ms_per_step": dtm * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u32",
            "data": "synthetic",
            "config": {"workload": "hash_to_point_prehashed_Fq2 of %d message hashes per GPU (SHA-256 chain, two SW encodings one per lane with the powers in registers, cofactor clearing one message per lane pair)" % n,
                       "name": "h2c", "check": check or "3 messages against the host integer code (itself pinned to the reference's vectors)"},
            "roofline": {"bound": "valu-int32-mac", "kernel": "k_pow + k_h2c_stage + k_h2c_clear", "peak": PEAK_TMACS, "unit": "TMAC/s",
                         "achieved": mac * n / dt / 1e12, "frac": mac * n / dt / 1e12 / PEAK_TMACS,
                         "traffic": config_traffic("h2c")[0] if n == 16384 else None, "traffic_source": config_traffic("h2c")[1] if n == 16384 else None,
                         "algorithmic_bytes": n * (32 + 192)}}
    return None


def dry_run(args):
    """what a test without a GPU can check of the multi-rank path: self-launch, rendezvous, the exchange"""
    import torch
    import torch.distributed as dist
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    got = [torch.full((144,), rank, dtype=torch.int32)]
    if world > 1:
        got = [torch.zeros(144, dtype=torch.int32) for _ in range(world)]
        with stdout_to_stderr():
            dist.init_process_group("gloo")
            dist.all_gather(got, torch.full((144,), rank, dtype=torch.int32))
            dist.barrier()
    if rank == 0:
        print(json.dumps({"dry_run": True, "n_gpus": world, "ranks_in_process_group": dist.get_world_size() if world > 1 else 1,
                          "partials_seen_from": [int(t[0]) for t in got]}))
    if world > 1:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed steps (default: 48 for c2 / c3, 3 for c4 / c5 / h2c)")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--config", default="c2", choices=["c2", "c3", "c4", "c5", "h2c"])
    ap.add_argument("--pairs", type=int, default=PAIRS_PER_GPU, help="c2: pairs per GPU per verification")
    ap.add_argument("--verifications", type=int, default=VERIFICATIONS_PER_STEP,
                    help="c2: independent aggregate verifications per step (one launch sequence)")
    ap.add_argument("--pairs-total", type=int, default=C3_PAIRS, help="c3: pairs of the one multi-pairing, over all GPUs")
    ap.add_argument("--groups", type=int, default=10000, help="c4: threshold groups per GPU")
    ap.add_argument("--points", type=int, default=1 << 20, help="c5: points per GPU")
    ap.add_argument("--messages", type=int, default=16384, help="h2c: messages per GPU")
    ap.add_argument("--streams", type=int, default=2,
                    help="steps in flight (the final exponentiations of one step overlap the Miller loops of the next)")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="gloo: CPU-side collective, for rehearsing the multi-rank path on one GPU")
    ap.add_argument("--force-process-group", action="store_true",
                    help="form the process group and run the all-gather even with one rank (RCCL rehearsal on a one-GPU box)")
    ap.add_argument("--free-streams", action="store_true",
                    help="do not order the Miller stages of consecutive steps (default: step i + 1's starts after step i's)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-peak-probe", action="store_true", help="skip the 30 ms multiply-add rate probe before the timed steps")
    ap.add_argument("--no-latency", action="store_true")
    ap.add_argument("--no-secondary", action="store_true", help="c2: skip the c3 / c4 / c5 / h2c runs after the timed region")
    ap.add_argument("--dry-run", action="store_true",
                    help="launch path only (no GPU): form the process group, all-gather one 576-byte partial per rank over gloo, report")
    ap.add_argument("--full", action="store_true",
                    help="c2 / c3: besides the timed steps, the result checks, the multiply-add probe and clock samples, the single-call "
                         "latencies, c3's 8-GPU projection, the CPU baselines and the secondary configs (the --no-* options thin this out)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="c2 / c3: write the results of the last timed step as DIR/<name>.npy (float32)")
    args = ap.parse_args()
    args.streams_given = any(a == "--streams" or a.startswith("--streams=") for a in sys.argv[1:])
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))
    if args.dry_run:
        return dry_run(args)
    if args.steps is None:
        args.steps = 3 if args.config in ("c4", "c5", "h2c") else 48
    if args.steps < 1:
        raise SystemExit("--steps must be at least 1")
    if args.dump_outputs and args.config not in ("c2", "c3"):
        raise SystemExit("--dump-outputs: c2 / c3 only")
    env = Env(args)
    if env.world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, env.world))
    line = {"c2": run_pairing, "c3": run_pairing, "c4": run_c4, "c5": run_c5, "h2c": run_h2c}[args.config](env, args)
    if line is not None:
        print(json.dumps(line))
    env.finish()


if __name__ == "__main__":
    main()
