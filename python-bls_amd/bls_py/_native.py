"""ctypes binding of libblsgpu.so (include/blsgpu.h) -- the HIP engine.

This is the product's only compute back-end for the pairing path.  There is no
CPU fallback: when the library or a GPU is missing, `engine()` raises.
"""
import array
import ctypes
import os
import sys
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(os.path.dirname(_HERE), "csrc", "libblsgpu.so")


class _Row(tuple):
    """a tuple that can carry .restype"""


def _returns(restype, *argtypes):
    """the PROTOTYPES row of a function that does not return int"""
    row = _Row(argtypes)
    row.restype = restype
    return row


vp, sz, cp, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_int

# Every function include/blsgpu.h declares, in the header's order: its argument types (tests/test_abi_and_host.py holds them
# against the header's declarations) and, by _returns, its return type where that is not int.  c_char_p: host bytes that
# Python hands in or a ctypes buffer; c_void_p: device pointers, streams and optional output buffers.
PROTOTYPES = {
    "blsgpu_version": _returns(cp),
    "blsgpu_last_error": _returns(cp),
    "blsgpu_ctx_create": (ci, ctypes.POINTER(vp)),
    "blsgpu_ctx_destroy": _returns(None, vp),
    "blsgpu_ctx_reserve": (vp, sz),
    "blsgpu_ctx_workspace_bytes": (vp, ctypes.POINTER(sz)),
    "blsgpu_ctx_trim": (vp,),
    "blsgpu_ctx_set_mp_threshold": (vp, sz),
    "blsgpu_timing_mad_probe": (vp, ctypes.c_double, ctypes.POINTER(ctypes.c_double), vp),
    "blsgpu_timing_mark": (vp, ctypes.c_uint, vp),
    "blsgpu_ctx_set_miller_wide_max": (vp, sz),
    "blsgpu_ctx_set_mp3_threshold": (vp, sz),
    "blsgpu_ctx_set_ls_threshold": (vp, sz, sz),
    "blsgpu_ctx_set_ls_teams": (vp, sz),
    "blsgpu_ctx_set_bulk_event": (vp, vp),
    "blsgpu_ctx_set_fexp_team_threshold": (vp, sz),
    "blsgpu_ctx_set_fexp_trace": (vp, vp),
    "blsgpu_ctx_set_fexpw_stamps": (vp, vp),
    "blsgpu_debug_read_lines": (vp, vp, sz),
    "blsgpu_verify_pipeline": (vp, cp, cp, cp, sz, cp, cp, cp, sz, cp),
    "blsgpu_verify_pipeline_dev": (vp, vp, vp, vp, sz, vp, vp, sz, vp, vp),
    "blsgpu_verify_aggregates": (vp, cp, cp, sz, cp, cp, sz, vp, vp, sz, vp, sz, vp, vp),
    "blsgpu_verify_aggregates_dev": (vp, vp, vp, sz, vp, vp, sz, vp, vp, sz, vp, sz, vp, vp, vp),
    "blsgpu_pairing_multi": (vp, cp, cp, cp, sz, cp),
    "blsgpu_pairing_multi_dev": (vp, vp, vp, vp, sz, vp, vp),
    "blsgpu_miller_loop_batch": (vp, cp, cp, cp, sz, cp),
    "blsgpu_miller_loop_batch_dev": (vp, vp, vp, vp, sz, vp, vp),
    "blsgpu_line_eval_batch": (vp, cp, cp, cp, sz, cp),
    "blsgpu_fq12_op_batch": (vp, ci, cp, cp, sz, cp),
    "blsgpu_fq12_pow_batch": (vp, cp, cp, sz, sz, cp),
    "blsgpu_miller_product_dev": (vp, vp, vp, vp, sz, vp, vp),
    "blsgpu_final_exp_product_dev": (vp, vp, sz, vp, vp),
    "blsgpu_final_exp": (vp, cp, cp),
    "blsgpu_final_exp_batch": (vp, cp, sz, cp),
    "blsgpu_pairing_multi_batch": (vp, cp, cp, cp, sz, sz, cp),
    "blsgpu_pairing_multi_batch_dev": (vp, vp, vp, vp, sz, sz, vp, vp),
    "blsgpu_miller_product_batch_dev": (vp, vp, vp, vp, sz, sz, vp, vp),
    "blsgpu_final_exp_product_batch_dev": (vp, vp, sz, sz, vp, vp),
    "blsgpu_g1_msm": (vp, cp, cp, sz, sz, cp, cp),
    "blsgpu_g2_msm": (vp, cp, cp, sz, sz, cp, cp),
    "blsgpu_g1_msm_dev": (vp, vp, vp, sz, sz, vp, vp, vp),
    "blsgpu_g2_msm_dev": (vp, vp, vp, sz, sz, vp, vp, vp),
    "blsgpu_map_to_g2": (vp, cp, sz, cp),
    "blsgpu_map_to_g2_dev": (vp, vp, sz, vp, vp),
    "blsgpu_hash_to_g2": (vp, cp, sz, cp),
    "blsgpu_hash_to_g2_dev": (vp, vp, sz, vp, vp),
    "blsgpu_map_to_g1": (vp, cp, sz, vp, vp, vp),
    "blsgpu_map_to_g1_dev": (vp, vp, sz, vp, vp, vp, vp),
    "blsgpu_hash_to_g1": (vp, cp, sz, vp, vp, vp),
    "blsgpu_hash_to_g1_dev": (vp, vp, sz, vp, vp, vp, vp),
    "blsgpu_g1_decompress": (vp, cp, sz, cp, cp),
    "blsgpu_g2_decompress": (vp, cp, sz, cp, cp),
    "blsgpu_g1_decompress_dev": (vp, vp, sz, vp, vp, vp),
    "blsgpu_g2_decompress_dev": (vp, vp, sz, vp, vp, vp),
    "blsgpu_g1_mul_gen": (vp, cp, sz, cp, sz, vp, vp),
    "blsgpu_g1_mul_gen_dev": (vp, vp, sz, vp, sz, vp, vp, vp),
    "blsgpu_g1_mul_gen_secret": (vp, cp, sz, vp, vp),
    "blsgpu_g1_mul_gen_secret_dev": (vp, vp, sz, vp, vp, vp),
    "blsgpu_hd_children": (vp, cp, cp, cp, vp, sz, vp, vp, vp, vp),
    "blsgpu_hd_children_dev": (vp, cp, cp, cp, vp, sz, vp, vp, vp, vp, vp),
    "blsgpu_hd_paths": (vp, cp, sz, ci, vp, vp, sz, sz, vp, vp, vp, vp, vp),
    "blsgpu_hd_paths_dev": (vp, vp, sz, ci, vp, vp, sz, sz, vp, vp, vp, vp, vp, vp),
    "blsgpu_hd_paths_secret": (vp, cp, sz, vp, vp, sz, sz, vp, vp, vp, vp, vp),
    "blsgpu_hd_paths_secret_dev": (vp, vp, sz, vp, vp, sz, sz, vp, vp, vp, vp, vp, vp),
    "blsgpu_keys_from_seeds": (vp, cp, sz, sz, ci, vp, vp, vp, vp, vp),
    "blsgpu_keys_from_seeds_dev": (vp, vp, sz, sz, ci, vp, vp, vp, vp, vp, vp),
    "blsgpu_g1_poly_check": (vp, cp, sz, sz, vp, cp, cp, sz, vp, vp),
    "blsgpu_g1_poly_check_dev": (vp, vp, sz, sz, vp, vp, vp, sz, vp, vp, vp),
    "blsgpu_g1_subgroup_check": (vp, cp, sz, vp),
    "blsgpu_g2_subgroup_check": (vp, cp, sz, vp),
    "blsgpu_g1_subgroup_check_dev": (vp, vp, sz, vp, vp),
    "blsgpu_g2_subgroup_check_dev": (vp, vp, sz, vp, vp),
    "blsgpu_lagrange_at_zero": (vp, cp, sz, sz, vp, vp),
    "blsgpu_lagrange_at_zero_dev": (vp, vp, sz, sz, vp, vp, vp),
    "blsgpu_fr_interpolate_at_zero": (vp, cp, cp, sz, sz, vp, vp),
    "blsgpu_fr_interpolate_at_zero_dev": (vp, vp, vp, sz, sz, vp, vp, vp),
    "blsgpu_threshold_combine": (vp, cp, cp, sz, sz, vp, vp, vp),
    "blsgpu_threshold_combine_dev": (vp, vp, vp, sz, sz, vp, vp, vp, vp),
    "blsgpu_sig_shares_check": (vp, cp, cp, sz, vp, cp, cp, cp, ci, sz, sz, vp, vp, vp),
    "blsgpu_sig_shares_check_dev": (vp, vp, vp, sz, vp, vp, vp, vp, ci, sz, sz, vp, vp, vp, vp),
    "blsgpu_g1_mul_short": (vp, cp, cp, sz, vp, vp),
    "blsgpu_g2_mul_short": (vp, cp, cp, sz, vp, vp),
    "blsgpu_g1_mul_short_dev": (vp, vp, vp, sz, vp, vp, vp),
    "blsgpu_g2_mul_short_dev": (vp, vp, vp, sz, vp, vp, vp),
    "blsgpu_verify_find": (vp, cp, cp, sz, vp, cp, sz, vp, cp, sz, vp, vp),
    "blsgpu_verify_find_dev": (vp, vp, vp, sz, vp, vp, sz, vp, vp, sz, vp, vp, vp),
    "blsgpu_g1_range_sums": (vp, cp, sz, vp, sz, vp, vp),
    "blsgpu_g2_range_sums": (vp, cp, sz, vp, sz, vp, vp),
    "blsgpu_g1_range_sums_dev": (vp, vp, sz, vp, sz, vp, vp, vp),
    "blsgpu_g2_range_sums_dev": (vp, vp, sz, vp, sz, vp, vp, vp),
    "blsgpu_g1_msm_ranges": (vp, cp, cp, sz, vp, sz, vp, vp),
    "blsgpu_g2_msm_ranges": (vp, cp, cp, sz, vp, sz, vp, vp),
    "blsgpu_g1_msm_ranges_dev": (vp, vp, vp, sz, vp, sz, vp, vp, vp),
    "blsgpu_g2_msm_ranges_dev": (vp, vp, vp, sz, vp, sz, vp, vp, vp),
    "blsgpu_pairing_multi_ranges": (vp, cp, cp, cp, sz, vp, sz, vp),
    "blsgpu_pairing_multi_ranges_dev": (vp, vp, vp, vp, sz, vp, sz, vp, vp),
    "blsgpu_sig_divide": (vp, cp, sz, vp, sz, vp, cp, cp, sz, vp, vp, vp, vp, vp),
    "blsgpu_sig_divide_dev": (vp, vp, sz, vp, sz, vp, vp, vp, sz, vp, vp, vp, vp, vp, vp),
    "blsgpu_verify_find_folded": (vp, cp, cp, sz, vp, cp, sz, vp, cp, sz, vp, vp),
    "blsgpu_verify_find_folded_dev": (vp, vp, vp, sz, vp, vp, sz, vp, vp, sz, vp, vp, vp),
    "blsgpu_g2_mul_secret": (vp, cp, sz, cp, sz, vp, vp, vp),
    "blsgpu_g2_mul_secret_dev": (vp, vp, sz, vp, sz, vp, vp, vp, vp),
    "blsgpu_sign": (vp, cp, cp, sz, sz, vp, vp),
    "blsgpu_sign_dev": (vp, vp, vp, sz, sz, vp, vp, vp),
    "blsgpu_threshold_deal_secret": (vp, cp, sz, sz, cp, sz, vp, vp),
    "blsgpu_threshold_deal_secret_dev": (vp, vp, sz, sz, vp, sz, vp, vp, vp),
    "blsgpu_fr_interpolate_at_zero_secret": (vp, cp, cp, sz, sz, vp, vp),
    "blsgpu_fr_interpolate_at_zero_secret_dev": (vp, vp, vp, sz, sz, vp, vp, vp),
    "blsgpu_g1_poly_check_secret": (vp, cp, sz, sz, vp, cp, cp, sz, vp, vp),
    "blsgpu_g1_poly_check_secret_dev": (vp, vp, sz, sz, vp, vp, vp, sz, vp, vp, vp),
    "blsgpu_fr_sum_secret": (vp, cp, sz, sz, vp, vp, vp),
    "blsgpu_fr_sum_secret_dev": (vp, vp, sz, sz, vp, vp, vp, vp),
    "blsgpu_sign_threshold": (vp, cp, cp, sz, sz, cp, sz, vp, vp, vp, vp),
    "blsgpu_sign_threshold_dev": (vp, vp, vp, sz, sz, vp, sz, vp, vp, vp, vp, vp),
    "blsgpu_hash_pks": (vp, cp, sz, sz, cp, sz, vp, vp),
    "blsgpu_hash_pks_dev": (vp, vp, sz, sz, vp, sz, vp, vp, vp),
    "blsgpu_aggregate_pub_keys_secure": (vp, cp, cp, cp, sz, sz, vp, vp),
    "blsgpu_aggregate_pub_keys_secure_dev": (vp, vp, vp, vp, sz, sz, vp, vp, vp),
    "blsgpu_aggregate_sigs_secure": (vp, cp, sz, cp, sz, cp, sz, vp, vp),
    "blsgpu_aggregate_sigs_secure_dev": (vp, vp, sz, vp, sz, vp, sz, vp, vp, vp),
    "blsgpu_aggregate_priv_keys_secure": (vp, cp, cp, cp, sz, sz, vp, vp, vp),
    "blsgpu_aggregate_priv_keys_secure_dev": (vp, vp, vp, vp, sz, sz, vp, vp, vp, vp),
    "blsgpu_hash_pks_ranges": (vp, cp, sz, vp, vp, sz, cp, vp, vp),
    "blsgpu_hash_pks_ranges_dev": (vp, vp, sz, vp, vp, sz, sz, vp, vp, vp, vp),
    "blsgpu_aggregate_pub_keys_secure_ranges": (vp, cp, cp, sz, vp, sz, cp, vp, vp),
    "blsgpu_aggregate_pub_keys_secure_ranges_dev": (vp, vp, vp, sz, vp, sz, vp, vp, vp, vp),
    "blsgpu_aggregate_sigs_secure_ranges": (vp, cp, sz, vp, cp, sz, vp, sz, cp, vp, vp),
    "blsgpu_aggregate_sigs_secure_ranges_dev": (vp, vp, sz, vp, vp, sz, vp, sz, vp, vp, vp, vp),
    "blsgpu_timing_enable": (vp, ci),
    "blsgpu_timing_read": (vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ci), sz, ctypes.POINTER(sz)),
}
del vp, sz, cp, ci

SYMBOLS = tuple(PROTOTYPES)

HD_PARENT_BYTES = 160          # BLSGPU_HD_PARENT_BYTES: chain code (32), public key affine (96), private key (32)
SEED_MAX_BYTES = 1024          # BLSGPU_SEED_MAX_BYTES: the longest seed blsgpu_keys_from_seeds takes
LAGRANGE_MAX_K = 1024          # BLSGPU_LAGRANGE_MAX_K of include/blsgpu.h: players per group the device takes
HASH_PKS_DEVICE_GROUPS = 64    # groups per call from which the device hashes the keys itself: below, one group per lane cannot
                               # fill a wavefront and the host's digest is handed in (pk_hash_in of include/blsgpu.h)

_lib = None
_lock = threading.Lock()


class BlsGpuError(RuntimeError):
    pass


def load_library(path=None):
    """dlopen libblsgpu.so and declare the prototypes (no GPU call is made)."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        p = path or os.environ.get("BLSGPU_LIBRARY", _LIB_PATH)
        # PyTorch-ROCm bundles its own HIP runtime.  If torch is going to be
        # used in this process (device buffers, streams, RCCL) it has to be
        # loaded first so that libblsgpu.so binds to the same runtime; loaded
        # the other way round torch no longer sees the GPU.
        if "torch" not in sys.modules and not os.environ.get("BLSGPU_NO_TORCH"):
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        if not os.path.exists(p):
            raise BlsGpuError("libblsgpu.so not found at %s -- run __graft_entry__.build() "
                              "(there is no CPU fallback)" % p)
        L = ctypes.CDLL(p)
        for name, row in PROTOTYPES.items():
            f = getattr(L, name)
            f.argtypes = list(row)
            f.restype = getattr(row, "restype", ctypes.c_int)
        _lib = L
        return L


class Engine:
    """One blsgpu context on one device."""

    def __init__(self, device=0):
        self.lib = load_library()
        h = ctypes.c_void_p()
        rc = self.lib.blsgpu_ctx_create(device, ctypes.byref(h))
        if rc != 0:
            raise BlsGpuError("blsgpu_ctx_create(%d) failed (%d): %s"
                              % (device, rc, self.lib.blsgpu_last_error().decode()))
        self.h = h
        self.device = device

    def _check(self, rc, what):
        if rc != 0:
            raise BlsGpuError("%s failed (%d): %s" % (what, rc, self.lib.blsgpu_last_error().decode()))

    def _call(self, name, *args):
        self._check(getattr(self.lib, name)(self.h, *args), name)

    def _call_out(self, name, *args, out, tail=()):
        """_call with output buffers after args (and `tail` after them): out holds a size in bytes per output, None for one
        that is not asked for (the library gets NULL).  -> the outputs' bytes, None likewise"""
        bufs = [None if size is None else ctypes.create_string_buffer(max(1, size)) for size in out]
        self._call(name, *args, *bufs, *tail)
        return [None if b is None else b.raw[:size] for b, size in zip(bufs, out)]

    @staticmethod
    def _scalars(v, n=None, what=None, width=32):
        """values of `width` (32 or 8) bytes big-endian each, from bytes or from ints below 2^(8 width); n: the count they
        must come to (None: the caller checks)"""
        b = bytes(v) if isinstance(v, (bytes, bytearray)) else b"".join(int(a).to_bytes(width, "big") for a in v)
        if n is not None and len(b) != width * n:
            raise ValueError("%s must hold k * groups values of %d bytes" % (what, width))
        return b

    @staticmethod
    def _flags(b):
        """[is_infinity] (or [accepted]) of the library's flag bytes"""
        return [c != 0 for c in b]

    @staticmethod
    def _indices(v, what):
        """a c_uint32 array of the indices v (of one zero for none: the pointer stays valid).  array("I") raises OverflowError
        outside 32 bits, where a c_uint32 array would wrap silently"""
        try:
            a = array.array("I", list(v) or [0])
        except OverflowError:
            raise OverflowError("%s indices are 32-bit" % what) from None
        return (ctypes.c_uint32 * len(a)).from_buffer(a)

    def close(self):
        if getattr(self, "h", None):
            self.lib.blsgpu_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def version(self):
        return self.lib.blsgpu_version().decode()

    def set_mp_threshold(self, pairs):
        """Batches >= pairs use the throughput kernel (several pairs per wavefront)."""
        self._call("blsgpu_ctx_set_mp_threshold", pairs)

    def mad_probe(self, target_ms=30.0, stream=None):
        """the chip's v_mad_i64_i32 rate right now, in 10^12 multiply-adds per second (a probe kernel of ~target_ms)"""
        out = ctypes.c_double(0.0)
        self._call("blsgpu_timing_mad_probe", float(target_ms), ctypes.byref(out), stream)
        return out.value

    def mark(self, tag=0, stream=None):
        """one dispatch of an empty kernel: brackets a timed region in a profile of the run"""
        self._call("blsgpu_timing_mark", tag, stream)

    def set_miller_wide_max(self, pairs):
        """Calls of at most `pairs` pairs run the wide Miller loop (one pair per two-wavefront workgroup); 0: never."""
        self._call("blsgpu_ctx_set_miller_wide_max", pairs)

    def set_mp3_threshold(self, pairs):
        """Throughput kernel: three pairs per wavefront from `pairs` pairs per call on, two below."""
        self._call("blsgpu_ctx_set_mp3_threshold", pairs)

    def set_ls_threshold(self, pairs, min_group=64):
        """Calls >= pairs with groups >= min_group use the line-stream kernels; pairs = None: never."""
        self._call("blsgpu_ctx_set_ls_threshold", (1 << 64) - 1 if pairs is None else pairs, min_group)

    WS_FIELDS = ("partials", "staging", "lines", "line_products", "flags_and_lists", "group_sums", "slots", "total")

    def workspace_bytes(self):
        """bytes of HBM the context's grow-only workspace holds, by purpose (include/blsgpu.h BLSGPU_WS_*)"""
        out = (ctypes.c_size_t * len(self.WS_FIELDS))()
        self._call("blsgpu_ctx_workspace_bytes", out)
        return dict(zip(self.WS_FIELDS, (int(v) for v in out)))

    def verify_pipeline(self, neg_g1, sig, hashes, n, keys_affine=None, key_pts=None, key_scalars=None, k=0):
        """e(-G1, sig) * prod_i e(P_i, H(m_i)) for n message hashes (32 bytes each): blsgpu_verify_pipeline -- ONE upload,
        then on the device hash-to-G2 of the hashes, P_i = either the given affine keys (n x 96 bytes) or the per-message
        key sums (key_pts: n x k x 96 bytes, key_scalars: n x k x 32 bytes big-endian) and the (n + 1)-pair
        multi-pairing; 576 bytes come back.  Host buffers and ctypes only: no torch."""
        out = ctypes.create_string_buffer(576)
        self._call("blsgpu_verify_pipeline", neg_g1, sig, hashes if n else None, n, keys_affine, key_pts, key_scalars, k, out)
        return out.raw

    def set_ls_teams(self, teams):
        self._call("blsgpu_ctx_set_ls_teams", teams)

    def set_fexp_team_threshold(self, results):
        """calls with >= results final exponentiations run them six lanes each; None: never"""
        self._call("blsgpu_ctx_set_fexp_team_threshold", (1 << 64) - 1 if results is None else results)

    def set_bulk_event(self, event_handle):
        """hipEvent_t handle (int; torch: event.cuda_event after a first record) recorded after the chip-filling
        kernels of every Miller stage, or None"""
        self._call("blsgpu_ctx_set_bulk_event", event_handle)

    def reserve(self, max_pairs):
        self._call("blsgpu_ctx_reserve", max_pairs)

    def trim(self):
        self._call("blsgpu_ctx_trim")

    @staticmethod
    def _inf(inf, n):
        """n x (P flag, Q flag) bytes, or None"""
        if inf is None:
            return None
        inf = bytes(inf)
        if len(inf) != 2 * n:
            raise ValueError("inf must hold 2 flags per pair")
        return inf

    def pairing_multi(self, g1: bytes, g2: bytes, n: int, inf=None) -> bytes:
        if len(g1) != 96 * n or len(g2) != 192 * n:
            raise ValueError("g1/g2 length does not match n")
        out = ctypes.create_string_buffer(576)
        self._call("blsgpu_pairing_multi", g1, g2, self._inf(inf, n), n, out)
        return out.raw

    def miller_loop_batch(self, g1: bytes, g2: bytes, n: int, inf=None) -> bytes:
        """n x 576 bytes: the reference's fq_miller_loop value of every pair."""
        if len(g1) != 96 * n or len(g2) != 192 * n:
            raise ValueError("g1/g2 length does not match n")
        return self._call_out("blsgpu_miller_loop_batch", g1, g2, self._inf(inf, n), n, out=[576 * n])[0]

    def line_eval_batch(self, r: bytes, q, p: bytes, n: int) -> bytes:
        """fq2_double_line_eval(R, P) (q None) / fq2_add_line_eval(R, Q, P) for n triples -> n x 576 bytes."""
        if len(r) != 192 * n or len(p) != 96 * n or (q is not None and len(q) != 192 * n):
            raise ValueError("buffer lengths do not match n")
        return self._call_out("blsgpu_line_eval_batch", r, q, p, n, out=[576 * n])[0]

    def final_exp(self, x: bytes) -> bytes:
        if len(x) != 576:
            raise ValueError("Fq12 must be 576 bytes")
        out = ctypes.create_string_buffer(576)
        self._call("blsgpu_final_exp", x, out)
        return out.raw

    def final_exp_batch(self, xs: bytes) -> bytes:
        if len(xs) % 576:
            raise ValueError("need m x 576 bytes")
        return self._call_out("blsgpu_final_exp_batch", xs, len(xs) // 576, out=[len(xs)])[0]

    FQ12_OPS = {"add": 0, "sub": 1, "mul": 2, "neg": 3, "inv": 4}

    def fq12_op(self, op: str, a: bytes, b: bytes = None) -> bytes:
        """fq12_add / sub / mul / neg / invert on n elements (n x 576 bytes each)."""
        if len(a) % 576 or (b is not None and len(b) != len(a)):
            raise ValueError("need n x 576 bytes")
        return self._call_out("blsgpu_fq12_op_batch", self.FQ12_OPS[op], a, b, len(a) // 576, out=[len(a)])[0]

    def fq12_pow(self, a: bytes, e: int) -> bytes:
        if len(a) % 576 or e < 0:
            raise ValueError("need n x 576 bytes and a non-negative exponent")
        eb = e.to_bytes(max(1, (e.bit_length() + 7) // 8), "big")
        return self._call_out("blsgpu_fq12_pow_batch", a, eb, len(eb), len(a) // 576, out=[len(a)])[0]

    def pairing_multi_batch(self, g1: bytes, g2: bytes, gsz: int, groups: int, inf=None) -> bytes:
        n = gsz * groups
        if len(g1) != 96 * n or len(g2) != 192 * n:
            raise ValueError("g1/g2 length does not match gsz * groups")
        return self._call_out("blsgpu_pairing_multi_batch", g1, g2, self._inf(inf, n), gsz, groups, out=[576 * groups])[0]

    def _decompress(self, name, insz, data):
        if len(data) % insz:
            raise ValueError("need n x %d bytes" % insz)
        k = len(data) // insz
        out, ok = self._call_out(name, data, k, out=[2 * len(data), k])
        return out, self._flags(ok)

    def g1_decompress(self, data: bytes):
        """n x 48 bytes -> (n x 96 bytes affine, [accepted])."""
        return self._decompress("blsgpu_g1_decompress", 48, data)

    def g2_decompress(self, data: bytes):
        """n x 96 bytes -> (n x 192 bytes affine, [accepted])."""
        return self._decompress("blsgpu_g2_decompress", 96, data)

    def hash_to_g2(self, msg_hashes: bytes) -> bytes:
        """n x 32-byte message hashes -> n x 192 bytes affine G2 (SHA-256 chain on the GPU too)."""
        if len(msg_hashes) % 32:
            raise ValueError("need n x 32 bytes")
        return self._call_out("blsgpu_hash_to_g2", msg_hashes, len(msg_hashes) // 32, out=[6 * len(msg_hashes)])[0]

    def map_to_g2(self, t: bytes) -> bytes:
        """t: n x 192 bytes (t0.c0, t0.c1, t1.c0, t1.c1) -> n x 192 bytes affine G2."""
        if len(t) % 192:
            raise ValueError("need n x 192 bytes")
        return self._call_out("blsgpu_map_to_g2", t, len(t) // 192, out=[len(t)])[0]

    def _msm(self, name, psz, pts, scalars, k, groups):
        n = k * groups
        if len(pts) != psz * n:
            raise ValueError("point buffer length does not match k * groups")
        sb = None
        if scalars is not None:
            sb = self._scalars(scalars)
            if len(sb) != 32 * n:
                raise ValueError("scalar buffer length does not match k * groups")
        out, inf = self._call_out(name, bytes(pts), sb, k, groups, out=[psz * groups, groups])
        return out, self._flags(inf)

    def g1_msm(self, pts, scalars, k, groups=1):
        """-> (groups x 96 affine bytes, [is_infinity])"""
        return self._msm("blsgpu_g1_msm", 96, pts, scalars, k, groups)

    def g2_msm(self, pts, scalars, k, groups=1):
        return self._msm("blsgpu_g2_msm", 192, pts, scalars, k, groups)

    def _mul_gen(self, name, scalars, add, aff, ser):
        """add: the (add, n_add) arguments of blsgpu_g1_mul_gen, checked here against the scalars; () for the secret form"""
        sb = self._scalars(scalars)
        if len(sb) % 32:
            raise ValueError("need n x 32 scalar bytes")
        n = len(sb) // 32
        if add and (add[1] not in (0, 1, n) or len(add[0] or b"") != 96 * add[1]):
            raise ValueError("add must hold 0, 1 or n points of 96 bytes")
        if not (aff or ser):
            raise ValueError("ask for at least one output")
        if add:
            add = (bytes(add[0]) if add[1] else None, add[1])
        return tuple(self._call_out(name, sb, n, *add, out=[96 * n if aff else None, 48 * n if ser else None]))

    def g1_mul_gen(self, scalars, add=None, n_add=0, aff=True, ser=True):
        """(s_i mod n) G1 (+ A) for n scalars (n x 32 bytes big-endian, or ints below 2^256) on the fixed-base table;
        add: None, one point (n_add = 1) or n points (n_add = n), 96 bytes affine each.
        -> (n x 96 affine bytes or None, n x 48 serialised bytes or None)"""
        return self._mul_gen("blsgpu_g1_mul_gen", scalars, (add, n_add), aff, ser)

    def g1_mul_gen_secret(self, scalars, aff=True, ser=True):
        """s_i G1 for n SECRET scalars (n x 32 bytes big-endian, or ints below 2^256) on the scalar-independent schedule of
        blsgpu_g1_mul_gen_secret; the bytes of g1_mul_gen.
        -> (n x 96 affine bytes or None, n x 48 serialised bytes or None)"""
        return self._mul_gen("blsgpu_g1_mul_gen_secret", scalars, (), aff, ser)

    def g1_mul_gen_secret_dev(self, d_scalars, n, d_out_aff, d_out_ser, stream=0):
        self._call("blsgpu_g1_mul_gen_secret_dev", d_scalars, n, d_out_aff, d_out_ser, stream)

    def hd_children(self, chain_code, parent_pk_aff, parent_sk, indices, aff=True, ser=True):
        """HD children of one parent (blsgpu_hd_children): parent_sk None = public derivation.
        -> (n x 32 chain codes, n x 32 child keys or None, n x 96 affine keys or None, n x 48 serialised keys or None)"""
        if len(chain_code) != 32 or len(parent_pk_aff) != 96 or (parent_sk is not None and len(parent_sk) != 32):
            raise ValueError("chain code 32, parent key 96 (and private key 32) bytes")
        n = len(indices)
        priv = parent_sk is not None
        return tuple(self._call_out("blsgpu_hd_children", bytes(chain_code), bytes(parent_pk_aff), bytes(parent_sk) if priv else None,
                                    self._indices(indices, "child"), n,
                                    out=[32 * n, 32 * n if priv else None, 96 * n if aff else None, 48 * n if ser else None]))

    def g1_mul_gen_dev(self, d_scalars, n, d_out_aff, d_out_ser, stream=0, d_add=None, n_add=0):
        self._call("blsgpu_g1_mul_gen_dev", d_scalars, n, d_add, n_add, d_out_aff, d_out_ser, stream)

    def hd_children_dev(self, chain_code, parent_pk_aff, parent_sk, d_indices, n, d_out_chain, d_out_sk, d_out_pk_aff,
                        d_out_pk_ser, stream=0):
        self._call("blsgpu_hd_children_dev", bytes(chain_code), bytes(parent_pk_aff), None if parent_sk is None else bytes(parent_sk),
                   d_indices, n, d_out_chain, d_out_sk, d_out_pk_aff, d_out_pk_ser, stream)

    def hd_paths_secret(self, parents, parent_of, paths, aff=True, ser=True, fp=True):
        """hd_paths in private mode on the scalar-independent schedule (blsgpu_hd_paths_secret): the same arguments without
        `priv`, the same outputs."""
        return self.hd_paths(parents, True, parent_of, paths, aff, ser, fp, secret=True)

    def hd_paths_secret_dev(self, d_parents, n_parents, d_parent_of, d_indices, depth, n, d_out_chain, d_out_sk, d_out_pk_aff,
                            d_out_pk_ser, d_out_parent_fp, stream=0):
        self._call("blsgpu_hd_paths_secret_dev", d_parents, n_parents, d_parent_of, d_indices, depth, n, d_out_chain, d_out_sk,
                   d_out_pk_aff, d_out_pk_ser, d_out_parent_fp, stream)

    def hd_paths(self, parents, priv, parent_of, paths, aff=True, ser=True, fp=True, secret=False):
        """HD paths of one depth, a parent per path (blsgpu_hd_paths).  parents: n_parents x 160 bytes (chain code, affine
        public key, private key or 32 zero bytes); priv: private derivation; parent_of: n indices into parents, or None
        (every path starts at parent 0); paths: n sequences of `depth` child indices each.
        -> (n x 32 chain codes, n x 32 keys or None (public), n x 96 affine keys or None, n x 48 serialised keys or None,
        n x 4 parent fingerprints or None), all of the paths' leaves"""
        if len(parents) % HD_PARENT_BYTES:
            raise ValueError("parent records are %d bytes" % HD_PARENT_BYTES)
        n = len(paths)
        depth = len(paths[0]) if n else 1
        if any(len(p) != depth for p in paths):
            raise ValueError("the paths of one call have one depth")
        if parent_of is not None and len(parent_of) != n:
            raise ValueError("one parent index per path")
        idx = self._indices([i for p in paths for i in p], "child")
        pof = None if parent_of is None else self._indices(parent_of, "parent")
        name, mode = ("blsgpu_hd_paths_secret", ()) if secret else ("blsgpu_hd_paths", (1 if priv else 0,))
        return tuple(self._call_out(name, bytes(parents), len(parents) // HD_PARENT_BYTES, *mode, pof, idx, depth, n,
                                    out=[32 * n, 32 * n if priv else None, 96 * n if aff else None, 48 * n if ser else None,
                                         4 * n if fp else None]))

    def hd_paths_dev(self, d_parents, n_parents, priv, d_parent_of, d_indices, depth, n, d_out_chain, d_out_sk, d_out_pk_aff,
                     d_out_pk_ser, d_out_parent_fp, stream=0):
        self._call("blsgpu_hd_paths_dev", d_parents, n_parents, 1 if priv else 0, d_parent_of, d_indices, depth, n, d_out_chain,
                   d_out_sk, d_out_pk_aff, d_out_pk_ser, d_out_parent_fp, stream)

    def g1_poly_check_secret(self, commit, n_polys, t, poly, x, s, aff=False):
        """g1_poly_check for SECRET fragments s on the scalar-independent schedule of blsgpu_g1_poly_check_secret: the same
        arguments (s is required: there is no evaluation-only mode), the same bytes.
        -> (n status bytes (1 equal, 0 not, 2 undecided), n x 96 affine Horner values or None)"""
        if s is None:
            raise ValueError("the secret form has no evaluation-only mode")
        return self.g1_poly_check(commit, n_polys, t, poly, x, s, aff, secret=True)

    def g1_poly_check_secret_dev(self, d_commit, n_polys, t, d_poly, d_x, d_s, n, d_status, d_out_aff, stream=0):
        self._call("blsgpu_g1_poly_check_secret_dev", d_commit, n_polys, t, d_poly, d_x, d_s, n, d_status, d_out_aff, stream)

    def g1_poly_check(self, commit, n_polys, t, poly, x, s=None, aff=False, secret=False):
        """Feldman share checks (blsgpu_g1_poly_check): commit n_polys x t x 96 affine bytes, poly n indices, x / s n x 32
        bytes big-endian (or ints below 2^256); s None = evaluation only.
        -> (n status bytes or None: 1 (s_i mod n) G1 == sum_k x_i^k C[poly_i][k], 0 not, 2 undecided -- poly_i has a C_k
        (k >= 1) outside the order-n subgroup; n x 96 affine Horner values or None)"""
        xb = self._scalars(x)
        n = len(poly)
        sb = None if s is None else self._scalars(s)
        if len(xb) != 32 * n or (sb is not None and len(sb) != 32 * n) or len(commit) != 96 * n_polys * t:
            raise ValueError("need n x 32 bytes of x (and s) and n_polys x t x 96 bytes of commitments")
        if sb is None and not aff:
            raise ValueError("ask for at least one output")
        return tuple(self._call_out("blsgpu_g1_poly_check_secret" if secret else "blsgpu_g1_poly_check", bytes(commit), n_polys, t,
                                    self._indices(poly, "polynomial"), xb, sb, n,
                                    out=[None if sb is None else n, 96 * n if aff else None]))

    def g1_poly_check_dev(self, d_commit, n_polys, t, d_poly, d_x, d_s, n, d_status, d_out_aff, stream=0):
        self._call("blsgpu_g1_poly_check_dev", d_commit, n_polys, t, d_poly, d_x, d_s, n, d_status, d_out_aff, stream)

    def _subgroup(self, name, psz, pts):
        if len(pts) % psz:
            raise ValueError("need n x %d bytes" % psz)
        n = len(pts) // psz
        return self._call_out(name, bytes(pts), n, out=[n])[0]

    def g1_subgroup(self, pts):
        """n x 96 affine bytes ((0, 0) = infinity) -> n status bytes: 1 in G1 (infinity included), 2 on the curve outside
        it, 0 off the curve"""
        return self._subgroup("blsgpu_g1_subgroup_check", 96, pts)

    def g2_subgroup(self, pts):
        """n x 192 affine bytes (all zero = infinity) -> n status bytes: 1 in G2 (infinity included), 2 on the twist
        outside it, 0 off it"""
        return self._subgroup("blsgpu_g2_subgroup_check", 192, pts)

    def g1_subgroup_dev(self, d_pts, n, d_status, stream=0):
        self._call("blsgpu_g1_subgroup_check_dev", d_pts, n, d_status, stream)

    def g2_subgroup_dev(self, d_pts, n, d_status, stream=0):
        self._call("blsgpu_g2_subgroup_check_dev", d_pts, n, d_status, stream)

    def lagrange_at_zero(self, x, k, groups=1):
        """Lagrange coefficients at zero of `groups` groups of k evaluation points (blsgpu_lagrange_at_zero): x
        groups x k x 32 bytes big-endian (or ints below 2^256), 1 <= k <= LAGRANGE_MAX_K.
        -> (groups x k x 32 coefficient bytes, groups status bytes: 1 written, 0 where the reference asserts -- zeros)"""
        n = k * groups
        return tuple(self._call_out("blsgpu_lagrange_at_zero", self._scalars(x, n, "x"), k, groups, out=[32 * n, groups]))

    def _interpolate(self, name, x, y, k, groups):
        n = k * groups
        return tuple(self._call_out(name, self._scalars(x, n, "x"), self._scalars(y, n, "y"), k, groups, out=[32 * groups, groups]))

    def fr_interpolate_at_zero(self, x, y, k, groups=1):
        """sum_j L_j y_j mod n per group (blsgpu_fr_interpolate_at_zero): x, y groups x k x 32 bytes big-endian (or ints
        below 2^256).  -> (groups x 32 bytes, groups status bytes)"""
        return self._interpolate("blsgpu_fr_interpolate_at_zero", x, y, k, groups)

    def threshold_combine(self, sigs, x, k, groups=1):
        """sum_j L_j sig_j per group (blsgpu_threshold_combine): sigs groups x k x 192 affine bytes, x as above.
        -> (groups x 192 affine bytes, [is_infinity], groups status bytes)"""
        n = k * groups
        if len(sigs) != 192 * n:
            raise ValueError("signature buffer length does not match k * groups")
        out, inf, st = self._call_out("blsgpu_threshold_combine", bytes(sigs), self._scalars(x, n, "x"), k, groups,
                                      out=[192 * groups, groups, groups])
        return out, self._flags(inf), st

    def lagrange_at_zero_dev(self, d_x, k, groups, d_out_coeffs, d_status, stream=0):
        self._call("blsgpu_lagrange_at_zero_dev", d_x, k, groups, d_out_coeffs, d_status, stream)

    def fr_interpolate_at_zero_dev(self, d_x, d_y, k, groups, d_out, d_status, stream=0):
        self._call("blsgpu_fr_interpolate_at_zero_dev", d_x, d_y, k, groups, d_out, d_status, stream)

    def threshold_combine_dev(self, d_sigs, d_x, k, groups, d_out, d_out_inf, d_status, stream=0):
        self._call("blsgpu_threshold_combine_dev", d_sigs, d_x, k, groups, d_out, d_out_inf, d_status, stream)

    def sig_shares_check(self, sigs, keys, key_idx, x, msg_hashes, weights, k, groups=1, scaled=True):
        """Signature shares of `groups` sessions of k shares checked on the device against their share public keys, a session
        by one random linear combination and the failing ones bisected (blsgpu_sig_shares_check): sigs groups x k x
        192 affine bytes, keys n_keys x 96 affine bytes, key_idx groups x k indices into them, x groups x k x 32 bytes
        big-endian (or ints below 2^256; None when not scaled), msg_hashes groups x 32 bytes, weights groups x k x 8 bytes
        big-endian (or ints below 2^64; a zero weight is taken as 1).
        -> (groups x k status bytes: 1 valid, 0 invalid, 2 not decided (the key is off the curve or outside G1); groups session
        status bytes: 0 where the player set is refused; (rounds, node tests))"""
        n = k * groups
        wb = self._scalars(weights, width=8)
        if len(sigs) != 192 * n or len(keys) % 96 or len(key_idx) != n or len(msg_hashes) != 32 * groups or len(wb) != 8 * n:
            raise ValueError("buffer lengths do not match k * groups")
        if scaled and x is None:
            raise ValueError("scaled shares need the player numbers")
        stats = (ctypes.c_uint64 * 2)()
        st, ss = self._call_out("blsgpu_sig_shares_check", bytes(sigs), bytes(keys), len(keys) // 96, self._indices(key_idx, "key"),
                                self._scalars(x, n, "x") if scaled else None, bytes(msg_hashes), wb, 1 if scaled else 0, k, groups,
                                out=[n, groups], tail=(stats,))
        return st, ss, (int(stats[0]), int(stats[1]))

    def sig_shares_check_dev(self, d_sigs, d_keys, n_keys, d_key_idx, d_x, d_msg_hashes, d_weights, scaled, k, groups, d_status,
                             d_session_status, stream=0):
        """-> (rounds, node tests); the status bytes are in d_status / d_session_status when the call returns"""
        stats = (ctypes.c_uint64 * 2)()
        self._call("blsgpu_sig_shares_check_dev", d_sigs, d_keys, n_keys, d_key_idx, d_x, d_msg_hashes, d_weights, 1 if scaled else 0,
                   k, groups, d_status, d_session_status, stats, stream)
        return int(stats[0]), int(stats[1])

    def g2_mul_secret(self, pts, scalars, aff=True, ser=True):
        """s_i P_i (or s_i P for ONE point of 192 bytes) for n scalars (n x 32 bytes big-endian, or ints below 2^256, taken as
        they are) on the scalar-independent schedule of blsgpu_g2_mul_secret.
        -> (n x 192 affine bytes or None, n x 96 serialised bytes or None, [is_infinity])"""
        sb = self._scalars(scalars)
        if len(sb) % 32 or len(pts) % 192:
            raise ValueError("need n x 32 scalar bytes and points of 192 bytes")
        n = len(sb) // 32
        if not (aff or ser):
            raise ValueError("ask for at least one output")
        oa, os_, inf = self._call_out("blsgpu_g2_mul_secret", bytes(pts), len(pts) // 192, sb, n,
                                      out=[192 * n if aff else None, 96 * n if ser else None, n])
        return oa, os_, self._flags(inf)

    def sign(self, sks, msg_hashes, aff=True, ser=True):
        """sk_i H(h_i) (or sk_i H(h) for ONE hash of 32 bytes) for n private keys (n x 32 bytes big-endian, or ints): the hash
        to G2 and the scalar-independent multiplication in one call (blsgpu_sign).
        -> (n x 192 affine bytes or None, n x 96 bytes of Signature.serialize() or None)"""
        sb = self._scalars(sks)
        if len(sb) % 32 or len(msg_hashes) % 32:
            raise ValueError("need n x 32 key bytes and hashes of 32 bytes")
        n = len(sb) // 32
        if not (aff or ser):
            raise ValueError("ask for at least one output")
        return tuple(self._call_out("blsgpu_sign", sb, bytes(msg_hashes), len(msg_hashes) // 32, n,
                                    out=[192 * n if aff else None, 96 * n if ser else None]))

    def g2_mul_secret_dev(self, d_pts, n_pts, d_scalars, n, d_out_aff, d_out_ser, d_out_inf=None, stream=0):
        self._call("blsgpu_g2_mul_secret_dev", d_pts, n_pts, d_scalars, n, d_out_aff, d_out_ser, d_out_inf, stream)

    def sign_dev(self, d_sks, d_msg_hashes, n_msg, n, d_out_aff, d_out_ser, stream=0):
        self._call("blsgpu_sign_dev", d_sks, d_msg_hashes, n_msg, n, d_out_aff, d_out_ser, stream)

    def threshold_deal_secret(self, coeffs, t, x, commit=True, frag=True):
        """Commitments and fragments of len(coeffs) / t polynomials with SECRET coefficients (blsgpu_threshold_deal_secret):
        coeffs n_polys x t x 32 bytes big-endian (or ints below 2^256), x the n_x points the fragments are taken at, likewise
        (ignored without frag).
        -> (n_polys x t x 96 affine bytes c_k G1 or None, n_polys x n_x x 32 bytes P_p(x_j) mod n or None)"""
        cb = self._scalars(coeffs)
        xb = self._scalars(x) if frag else b""
        if t < 1 or len(cb) % (32 * t) or len(xb) % 32:
            raise ValueError("need n_polys x t x 32 coefficient bytes and n_x x 32 bytes of points")
        if not (commit or frag):
            raise ValueError("ask for at least one output")
        n_polys, n_x = len(cb) // (32 * t), len(xb) // 32
        return tuple(self._call_out("blsgpu_threshold_deal_secret", cb, n_polys, t, xb if frag else None, n_x,
                                    out=[96 * n_polys * t if commit else None, 32 * n_polys * n_x if frag else None]))

    def threshold_deal_secret_dev(self, d_coeffs, n_polys, t, d_x, n_x, d_out_commit_aff, d_out_frag, stream=0):
        self._call("blsgpu_threshold_deal_secret_dev", d_coeffs, n_polys, t, d_x, n_x, d_out_commit_aff, d_out_frag, stream)

    def fr_interpolate_at_zero_secret(self, x, y, k, groups=1):
        """fr_interpolate_at_zero for SECRET y (shares) on the masked sums of blsgpu_fr_interpolate_at_zero_secret: the same
        arguments, the same bytes.  -> (groups x 32 bytes, groups status bytes)"""
        return self._interpolate("blsgpu_fr_interpolate_at_zero_secret", x, y, k, groups)

    def fr_interpolate_at_zero_secret_dev(self, d_x, d_y, k, groups, d_out, d_status, stream=0):
        self._call("blsgpu_fr_interpolate_at_zero_secret_dev", d_x, d_y, k, groups, d_out, d_status, stream)

    def _secret_sum(self, name, *args, groups, pk, aff, ser):
        """-> (groups x 32 bytes of sums, groups x 96 affine bytes of their public keys (aff or pk) or None, groups x 48
        serialised bytes (ser or pk) or None)"""
        return tuple(self._call_out(name, *args, groups, out=[32 * groups, 96 * groups if aff or pk else None,
                                                              48 * groups if ser or pk else None]))

    def fr_sum_secret(self, y, k, groups=1, pk=False, aff=False, ser=False):
        """sum_j y_j mod n per group for SECRET y (blsgpu_fr_sum_secret: a player's share from the fragments it was dealt): y
        groups x k x 32 bytes big-endian (or ints below 2^256), k >= 1.  pk: both forms of the public key of every sum
        (aff / ser: one of them), multiplied on the device by k_fix_mul_secret.
        -> (groups x 32 bytes, groups x 96 affine bytes or None, groups x 48 serialised bytes or None)"""
        if k < 1:
            raise ValueError("k must be at least 1")
        return self._secret_sum("blsgpu_fr_sum_secret", self._scalars(y, k * groups, "y"), k, groups=groups, pk=pk, aff=aff, ser=ser)

    def fr_sum_secret_dev(self, d_y, k, groups, d_out, d_out_pk_aff, d_out_pk_ser, stream=0):
        self._call("blsgpu_fr_sum_secret_dev", d_y, k, groups, d_out, d_out_pk_aff, d_out_pk_ser, stream)

    def sign_threshold(self, sks, x, k, msg_hashes, groups=1, aff=True, ser=True):
        """Unit signatures (lambda_j sk_j mod n) H(h) of `groups` sessions of k signers (blsgpu_sign_threshold): sks, x
        groups x k x 32 bytes big-endian (or ints below 2^256), msg_hashes ONE hash of 32 bytes or one per session.
        -> (groups x k x 192 affine bytes or None, groups x k x 96 serialised bytes or None, [is_infinity], groups status bytes)"""
        n = k * groups
        if len(msg_hashes) % 32:
            raise ValueError("message hashes are 32 bytes")
        if not (aff or ser):
            raise ValueError("ask for at least one output")
        oa, os_, inf, st = self._call_out("blsgpu_sign_threshold", self._scalars(sks, n, "sks"), self._scalars(x, n, "x"), k, groups,
                                          bytes(msg_hashes), len(msg_hashes) // 32,
                                          out=[192 * n if aff else None, 96 * n if ser else None, n, groups])
        return oa, os_, self._flags(inf), st

    def sign_threshold_dev(self, d_sks, d_x, k, groups, d_msg_hashes, n_msg, d_out_aff, d_out_ser, d_out_inf, d_status, stream=0):
        self._call("blsgpu_sign_threshold_dev", d_sks, d_x, k, groups, d_msg_hashes, n_msg, d_out_aff, d_out_ser, d_out_inf, d_status,
                   stream)

    # ---- secure aggregation: the hash_pks exponents on the device and the three sums behind them ----
    @staticmethod
    def _pk_hashes(pks_ser, k, groups, pk_hash):
        """the pk_hash_in of a call: the caller's digests, the host's for fewer than HASH_PKS_DEVICE_GROUPS groups (one group
        per lane cannot fill a wavefront; hashlib runs at memory speed), or None: the device hashes the keys.
        pk_hash: bytes, None (that rule) or False (the device, whatever the count)"""
        if len(pks_ser) != 48 * k * groups:
            raise ValueError("need groups x k serialised keys of 48 bytes")
        if pk_hash is False or (pk_hash is None and groups >= HASH_PKS_DEVICE_GROUPS):
            return None
        if pk_hash is None:
            import hashlib
            mv = memoryview(pks_ser)
            return b"".join(hashlib.sha256(mv[48 * k * g:48 * k * (g + 1)]).digest() for g in range(groups))
        if len(pk_hash) != 32 * groups:
            raise ValueError("need one digest of 32 bytes per group")
        return bytes(pk_hash)

    def hash_pks(self, pks_ser, k, m, groups=1, pk_hash=None, want_pk_hash=False):
        """util.hash_pks(m, keys) of `groups` groups of k serialised keys (blsgpu_hash_pks): groups x m exponents below n,
        t_i = sha256(be32(i) || sha256(the group's k serialised keys)) mod n, 32 bytes big-endian each.  pk_hash: see
        _pk_hashes.  -> exponent bytes (, groups x 32 digest bytes)"""
        pks_ser = bytes(pks_ser)
        ph = self._pk_hashes(pks_ser, k, groups, pk_hash)
        out, dg = self._call_out("blsgpu_hash_pks", None if ph else pks_ser, k, groups, ph, m,
                                 out=[32 * m * groups, 32 * groups if want_pk_hash else None])
        return (out, dg) if want_pk_hash else out

    def _aggregate_secure(self, name, psz, what, pts, k, pks_ser, k_pks, groups, pk_hash, args):
        """args(pts, pks_ser or None, digests or None): the call's arguments before `groups`"""
        pks_ser = bytes(pks_ser)
        if len(pts) != psz * k * groups:
            raise ValueError("%s buffer length does not match k * groups" % what)
        ph = self._pk_hashes(pks_ser, k_pks, groups, pk_hash)
        out, inf = self._call_out(name, *args(bytes(pts), None if ph else pks_ser, ph), groups, out=[psz * groups, groups])
        return out, self._flags(inf)

    def aggregate_pub_keys_secure(self, pts_aff, pks_ser, k, groups=1, pk_hash=None):
        """sum_i t_i P_i per group (blsgpu_aggregate_pub_keys_secure): pts_aff groups x k x 96 affine bytes, pks_ser the same
        keys serialised, both in the order to be hashed.  -> (groups x 96 affine bytes, [is_infinity])"""
        return self._aggregate_secure("blsgpu_aggregate_pub_keys_secure", 96, "point", pts_aff, k, pks_ser, k, groups, pk_hash,
                                      lambda pts, pks, ph: (pts, pks, ph, k))

    def aggregate_sigs_secure(self, sigs_aff, k, pks_ser, k_pks, groups=1, pk_hash=None):
        """sum_i t_i S_i per group (blsgpu_aggregate_sigs_secure): sigs_aff groups x k x 192 affine bytes in the order the
        exponents multiply them, the k exponents hashed over k_pks serialised keys per group.
        -> (groups x 192 affine bytes, [is_infinity])"""
        return self._aggregate_secure("blsgpu_aggregate_sigs_secure", 192, "signature", sigs_aff, k, pks_ser, k_pks, groups, pk_hash,
                                      lambda sigs, pks, ph: (sigs, k, pks, k_pks, ph))

    def aggregate_priv_keys_secure(self, sks, pks_ser, k, groups=1, pk=False, aff=False, ser=False, pk_hash=None):
        """sum_i t_i sk_i mod n per group for SECRET keys (blsgpu_aggregate_priv_keys_secure): sks groups x k x 32 bytes
        big-endian (or ints below 2^256) in the order the exponents multiply them, pks_ser in the order to be hashed,
        1 <= k <= LAGRANGE_MAX_K.  pk: both forms of the public key of every sum (aff / ser: one of them).
        -> (groups x 32 bytes, groups x 96 affine bytes or None, groups x 48 serialised bytes or None)"""
        pks_ser = bytes(pks_ser)
        ph = self._pk_hashes(pks_ser, k, groups, pk_hash)
        return self._secret_sum("blsgpu_aggregate_priv_keys_secure", self._scalars(sks, k * groups, "sks"), None if ph else pks_ser, ph, k,
                                groups=groups, pk=pk, aff=aff, ser=ser)

    def hash_pks_dev(self, d_pks_ser, k, groups, d_pk_hash_in, m, d_out_ts, d_out_pk_hash=None, stream=0):
        self._call("blsgpu_hash_pks_dev", d_pks_ser, k, groups, d_pk_hash_in, m, d_out_ts, d_out_pk_hash, stream)

    def aggregate_pub_keys_secure_dev(self, d_pts_aff, d_pks_ser, d_pk_hash_in, k, groups, d_out_aff, d_out_inf=None, stream=0):
        self._call("blsgpu_aggregate_pub_keys_secure_dev", d_pts_aff, d_pks_ser, d_pk_hash_in, k, groups, d_out_aff, d_out_inf, stream)

    def aggregate_sigs_secure_dev(self, d_sigs_aff, k, d_pks_ser, k_pks, d_pk_hash_in, groups, d_out_aff, d_out_inf=None, stream=0):
        self._call("blsgpu_aggregate_sigs_secure_dev", d_sigs_aff, k, d_pks_ser, k_pks, d_pk_hash_in, groups, d_out_aff, d_out_inf, stream)

    def aggregate_priv_keys_secure_dev(self, d_sks, d_pks_ser, d_pk_hash_in, k, groups, d_out, d_out_pk_aff=None, d_out_pk_ser=None, stream=0):
        self._call("blsgpu_aggregate_priv_keys_secure_dev", d_sks, d_pks_ser, d_pk_hash_in, k, groups, d_out, d_out_pk_aff, d_out_pk_ser,
                   stream)

    def timing_enable(self, on=True):
        self._call("blsgpu_timing_enable", int(on))

    def timing_read(self):
        """[(kind, ms)] for every kernel launched since the last read; kinds:
        0 k_miller, 1 k_reduce, 2 k_reduce + final exponentiation, 3 k_miller_slow (the rest: include/blsgpu.h)."""
        cap = 1024
        ms = (ctypes.c_float * cap)()
        kind = (ctypes.c_int * cap)()
        cnt = ctypes.c_size_t(0)
        self._call("blsgpu_timing_read", ms, kind, cap, ctypes.byref(cnt))
        return [(kind[i], ms[i]) for i in range(cnt.value)]

    # device-pointer forms (integers: tensor.data_ptr(), stream.cuda_stream)
    # (d_inf: device pointer to n x 2 flag bytes, or None)
    def pairing_multi_dev(self, d_g1, d_g2, n, d_out, stream=0, d_inf=None):
        self._call("blsgpu_pairing_multi_dev", d_g1, d_g2, d_inf, n, d_out, stream)

    def miller_loop_batch_dev(self, d_g1, d_g2, n, d_out, stream=0, d_inf=None):
        self._call("blsgpu_miller_loop_batch_dev", d_g1, d_g2, d_inf, n, d_out, stream)

    def miller_product_dev(self, d_g1, d_g2, n, d_partial, stream=0, d_inf=None):
        self._call("blsgpu_miller_product_dev", d_g1, d_g2, d_inf, n, d_partial, stream)

    def final_exp_product_dev(self, d_partials, m, d_out, stream=0):
        self._call("blsgpu_final_exp_product_dev", d_partials, m, d_out, stream)

    def pairing_multi_batch_dev(self, d_g1, d_g2, gsz, groups, d_out, stream=0, d_inf=None):
        self._call("blsgpu_pairing_multi_batch_dev", d_g1, d_g2, d_inf, gsz, groups, d_out, stream)

    def miller_product_batch_dev(self, d_g1, d_g2, gsz, groups, d_partials, stream=0, d_inf=None):
        self._call("blsgpu_miller_product_batch_dev", d_g1, d_g2, d_inf, gsz, groups, d_partials, stream)

    def final_exp_product_batch_dev(self, d_partials, m, groups, d_out, stream=0):
        self._call("blsgpu_final_exp_product_batch_dev", d_partials, m, groups, d_out, stream)


_engines = {}


def engine(device=0):
    """Process-wide engine for `device`; raises BlsGpuError if unavailable."""
    with _lock:
        e = _engines.get(device)
    if e is None:
        e = Engine(device)
        with _lock:
            _engines[device] = e
    return e
