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

SYMBOLS = (
    "blsgpu_version", "blsgpu_last_error", "blsgpu_ctx_create", "blsgpu_ctx_destroy",
    "blsgpu_ctx_reserve", "blsgpu_ctx_set_mp_threshold", "blsgpu_ctx_set_miller_wide_max", "blsgpu_pairing_multi", "blsgpu_pairing_multi_dev",
    "blsgpu_miller_product_dev", "blsgpu_final_exp_product_dev", "blsgpu_final_exp",
    "blsgpu_timing_enable", "blsgpu_timing_read", "blsgpu_timing_mad_probe", "blsgpu_timing_mark",
    "blsgpu_g1_msm", "blsgpu_g2_msm", "blsgpu_g1_msm_dev", "blsgpu_g2_msm_dev",
    "blsgpu_final_exp_batch", "blsgpu_pairing_multi_batch", "blsgpu_pairing_multi_batch_dev",
    "blsgpu_map_to_g2", "blsgpu_map_to_g2_dev",
    "blsgpu_miller_product_batch_dev", "blsgpu_final_exp_product_batch_dev",
    "blsgpu_g1_decompress", "blsgpu_g2_decompress", "blsgpu_g1_decompress_dev", "blsgpu_g2_decompress_dev",
    "blsgpu_hash_to_g2", "blsgpu_hash_to_g2_dev",
    "blsgpu_miller_loop_batch", "blsgpu_miller_loop_batch_dev", "blsgpu_line_eval_batch", "blsgpu_ctx_trim",
    "blsgpu_fq12_op_batch", "blsgpu_fq12_pow_batch", "blsgpu_ctx_set_mp3_threshold", "blsgpu_ctx_set_ls_threshold", "blsgpu_ctx_set_ls_teams", "blsgpu_ctx_set_bulk_event", "blsgpu_ctx_set_fexp_team_threshold", "blsgpu_ctx_set_fexp_trace", "blsgpu_ctx_set_fexpw_stamps", "blsgpu_debug_read_lines",
    "blsgpu_ctx_workspace_bytes", "blsgpu_verify_pipeline", "blsgpu_verify_pipeline_dev",
    "blsgpu_g1_mul_gen", "blsgpu_g1_mul_gen_dev", "blsgpu_hd_children", "blsgpu_hd_children_dev",
    "blsgpu_hd_paths", "blsgpu_hd_paths_dev",
    "blsgpu_g1_poly_check", "blsgpu_g1_poly_check_dev",
    "blsgpu_g1_subgroup_check", "blsgpu_g1_subgroup_check_dev", "blsgpu_g2_subgroup_check", "blsgpu_g2_subgroup_check_dev",
    "blsgpu_lagrange_at_zero", "blsgpu_lagrange_at_zero_dev", "blsgpu_fr_interpolate_at_zero", "blsgpu_fr_interpolate_at_zero_dev",
    "blsgpu_threshold_combine", "blsgpu_threshold_combine_dev", "blsgpu_sig_shares_check", "blsgpu_sig_shares_check_dev",
    "blsgpu_g2_mul_secret", "blsgpu_g2_mul_secret_dev", "blsgpu_sign", "blsgpu_sign_dev",
    "blsgpu_g1_mul_gen_secret", "blsgpu_g1_mul_gen_secret_dev", "blsgpu_hd_paths_secret", "blsgpu_hd_paths_secret_dev",
    "blsgpu_threshold_deal_secret", "blsgpu_threshold_deal_secret_dev",
    "blsgpu_fr_interpolate_at_zero_secret", "blsgpu_fr_interpolate_at_zero_secret_dev",
    "blsgpu_sign_threshold", "blsgpu_sign_threshold_dev",
    "blsgpu_g1_poly_check_secret", "blsgpu_g1_poly_check_secret_dev", "blsgpu_fr_sum_secret", "blsgpu_fr_sum_secret_dev",
    "blsgpu_hash_pks", "blsgpu_hash_pks_dev", "blsgpu_aggregate_pub_keys_secure", "blsgpu_aggregate_pub_keys_secure_dev",
    "blsgpu_aggregate_sigs_secure", "blsgpu_aggregate_sigs_secure_dev",
    "blsgpu_aggregate_priv_keys_secure", "blsgpu_aggregate_priv_keys_secure_dev",
)

HD_PARENT_BYTES = 160          # BLSGPU_HD_PARENT_BYTES: chain code (32), public key affine (96), private key (32)
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
        vp, sz, cp = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p
        L.blsgpu_version.restype = cp
        L.blsgpu_last_error.restype = cp
        L.blsgpu_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
        L.blsgpu_ctx_destroy.argtypes = [vp]
        L.blsgpu_ctx_destroy.restype = None
        L.blsgpu_ctx_reserve.argtypes = [vp, sz]
        L.blsgpu_ctx_set_mp_threshold.argtypes = [vp, sz]
        L.blsgpu_ctx_set_mp3_threshold.argtypes = [vp, sz]
        L.blsgpu_timing_mad_probe.argtypes = [vp, ctypes.c_double, ctypes.POINTER(ctypes.c_double), vp]
        L.blsgpu_timing_mark.argtypes = [vp, ctypes.c_uint, vp]
        L.blsgpu_ctx_set_miller_wide_max.argtypes = [vp, sz]
        L.blsgpu_ctx_set_ls_threshold.argtypes = [vp, sz, sz]
        L.blsgpu_ctx_set_ls_teams.argtypes = [vp, sz]
        L.blsgpu_ctx_set_bulk_event.argtypes = [vp, vp]
        L.blsgpu_ctx_set_fexp_team_threshold.argtypes = [vp, sz]
        L.blsgpu_ctx_set_fexp_trace.argtypes = [vp, vp]
        L.blsgpu_ctx_set_fexpw_stamps.argtypes = [vp, vp]
        L.blsgpu_debug_read_lines.argtypes = [vp, vp, sz]
        L.blsgpu_ctx_workspace_bytes.argtypes = [vp, ctypes.POINTER(ctypes.c_size_t)]
        L.blsgpu_verify_pipeline.argtypes = [vp, cp, cp, cp, sz, cp, cp, cp, sz, cp]
        L.blsgpu_verify_pipeline_dev.argtypes = [vp, vp, vp, vp, sz, vp, vp, sz, vp, vp]
        L.blsgpu_ctx_trim.argtypes = [vp]
        L.blsgpu_pairing_multi.argtypes = [vp, cp, cp, cp, sz, cp]
        L.blsgpu_pairing_multi_dev.argtypes = [vp, vp, vp, vp, sz, vp, vp]
        L.blsgpu_miller_loop_batch.argtypes = [vp, cp, cp, cp, sz, cp]
        L.blsgpu_miller_loop_batch_dev.argtypes = [vp, vp, vp, vp, sz, vp, vp]
        L.blsgpu_line_eval_batch.argtypes = [vp, cp, cp, cp, sz, cp]
        L.blsgpu_fq12_op_batch.argtypes = [vp, ctypes.c_int, cp, cp, sz, cp]
        L.blsgpu_fq12_pow_batch.argtypes = [vp, cp, cp, sz, sz, cp]
        L.blsgpu_miller_product_dev.argtypes = [vp, vp, vp, vp, sz, vp, vp]
        L.blsgpu_final_exp_product_dev.argtypes = [vp, vp, sz, vp, vp]
        L.blsgpu_final_exp.argtypes = [vp, cp, cp]
        for f in (L.blsgpu_g1_msm, L.blsgpu_g2_msm):
            f.argtypes = [vp, cp, cp, sz, sz, cp, cp]
        for f in (L.blsgpu_g1_msm_dev, L.blsgpu_g2_msm_dev):
            f.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp]
        L.blsgpu_final_exp_batch.argtypes = [vp, cp, sz, cp]
        L.blsgpu_pairing_multi_batch.argtypes = [vp, cp, cp, cp, sz, sz, cp]
        L.blsgpu_pairing_multi_batch_dev.argtypes = [vp, vp, vp, vp, sz, sz, vp, vp]
        L.blsgpu_miller_product_batch_dev.argtypes = [vp, vp, vp, vp, sz, sz, vp, vp]
        L.blsgpu_final_exp_product_batch_dev.argtypes = [vp, vp, sz, sz, vp, vp]
        L.blsgpu_g1_decompress.argtypes = [vp, cp, sz, cp, cp]
        L.blsgpu_g2_decompress.argtypes = [vp, cp, sz, cp, cp]
        L.blsgpu_g1_decompress_dev.argtypes = [vp, vp, sz, vp, vp, vp]
        L.blsgpu_g2_decompress_dev.argtypes = [vp, vp, sz, vp, vp, vp]
        L.blsgpu_hash_to_g2.argtypes = [vp, cp, sz, cp]
        L.blsgpu_hash_to_g2_dev.argtypes = [vp, vp, sz, vp, vp]
        L.blsgpu_map_to_g2.argtypes = [vp, cp, sz, cp]
        L.blsgpu_map_to_g2_dev.argtypes = [vp, vp, sz, vp, vp]
        L.blsgpu_g1_mul_gen.argtypes = [vp, cp, sz, cp, sz, vp, vp]
        L.blsgpu_g1_mul_gen_dev.argtypes = [vp, vp, sz, vp, sz, vp, vp, vp]
        L.blsgpu_hd_children.argtypes = [vp, cp, cp, cp, vp, sz, vp, vp, vp, vp]
        L.blsgpu_hd_children_dev.argtypes = [vp, cp, cp, cp, vp, sz, vp, vp, vp, vp, vp]
        L.blsgpu_hd_paths.argtypes = [vp, cp, sz, ctypes.c_int, vp, vp, sz, sz, vp, vp, vp, vp, vp]
        L.blsgpu_hd_paths_dev.argtypes = [vp, vp, sz, ctypes.c_int, vp, vp, sz, sz, vp, vp, vp, vp, vp, vp]
        L.blsgpu_g1_poly_check.argtypes = [vp, cp, sz, sz, vp, cp, cp, sz, vp, vp]
        L.blsgpu_g1_poly_check_dev.argtypes = [vp, vp, sz, sz, vp, vp, vp, sz, vp, vp, vp]
        for g in ("g1", "g2"):
            getattr(L, "blsgpu_%s_subgroup_check" % g).argtypes = [vp, cp, sz, vp]
            getattr(L, "blsgpu_%s_subgroup_check_dev" % g).argtypes = [vp, vp, sz, vp, vp]
        L.blsgpu_lagrange_at_zero.argtypes = [vp, cp, sz, sz, vp, vp]
        L.blsgpu_lagrange_at_zero_dev.argtypes = [vp, vp, sz, sz, vp, vp, vp]
        L.blsgpu_fr_interpolate_at_zero.argtypes = [vp, cp, cp, sz, sz, vp, vp]
        L.blsgpu_fr_interpolate_at_zero_dev.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp]
        L.blsgpu_threshold_combine.argtypes = [vp, cp, cp, sz, sz, vp, vp, vp]
        L.blsgpu_threshold_combine_dev.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp, vp]
        L.blsgpu_sig_shares_check.argtypes = [vp, cp, cp, sz, vp, cp, cp, cp, ctypes.c_int, sz, sz, vp, vp, vp]
        L.blsgpu_sig_shares_check_dev.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp, ctypes.c_int, sz, sz, vp, vp, vp, vp]
        L.blsgpu_g2_mul_secret.argtypes = [vp, cp, sz, cp, sz, vp, vp, vp]
        L.blsgpu_g2_mul_secret_dev.argtypes = [vp, vp, sz, vp, sz, vp, vp, vp, vp]
        L.blsgpu_sign.argtypes = [vp, cp, cp, sz, sz, vp, vp]
        L.blsgpu_sign_dev.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp]
        L.blsgpu_g1_mul_gen_secret.argtypes = [vp, cp, sz, vp, vp]
        L.blsgpu_g1_mul_gen_secret_dev.argtypes = [vp, vp, sz, vp, vp, vp]
        L.blsgpu_hd_paths_secret.argtypes = [vp, cp, sz, vp, vp, sz, sz, vp, vp, vp, vp, vp]
        L.blsgpu_hd_paths_secret_dev.argtypes = [vp, vp, sz, vp, vp, sz, sz, vp, vp, vp, vp, vp, vp]
        L.blsgpu_threshold_deal_secret.argtypes = [vp, cp, sz, sz, cp, sz, vp, vp]
        L.blsgpu_threshold_deal_secret_dev.argtypes = [vp, vp, sz, sz, vp, sz, vp, vp, vp]
        L.blsgpu_fr_interpolate_at_zero_secret.argtypes = [vp, cp, cp, sz, sz, vp, vp]
        L.blsgpu_fr_interpolate_at_zero_secret_dev.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp]
        L.blsgpu_sign_threshold.argtypes = [vp, cp, cp, sz, sz, cp, sz, vp, vp, vp, vp]
        L.blsgpu_sign_threshold_dev.argtypes = [vp, vp, vp, sz, sz, vp, sz, vp, vp, vp, vp, vp]
        L.blsgpu_g1_poly_check_secret.argtypes = [vp, cp, sz, sz, vp, cp, cp, sz, vp, vp]
        L.blsgpu_g1_poly_check_secret_dev.argtypes = [vp, vp, sz, sz, vp, vp, vp, sz, vp, vp, vp]
        L.blsgpu_fr_sum_secret.argtypes = [vp, cp, sz, sz, vp, vp, vp]
        L.blsgpu_fr_sum_secret_dev.argtypes = [vp, vp, sz, sz, vp, vp, vp, vp]
        L.blsgpu_hash_pks.argtypes = [vp, cp, sz, sz, cp, sz, vp, vp]
        L.blsgpu_hash_pks_dev.argtypes = [vp, vp, sz, sz, vp, sz, vp, vp, vp]
        L.blsgpu_aggregate_pub_keys_secure.argtypes = [vp, cp, cp, cp, sz, sz, vp, vp]
        L.blsgpu_aggregate_pub_keys_secure_dev.argtypes = [vp, vp, vp, vp, sz, sz, vp, vp, vp]
        L.blsgpu_aggregate_sigs_secure.argtypes = [vp, cp, sz, cp, sz, cp, sz, vp, vp]
        L.blsgpu_aggregate_sigs_secure_dev.argtypes = [vp, vp, sz, vp, sz, vp, sz, vp, vp, vp]
        L.blsgpu_aggregate_priv_keys_secure.argtypes = [vp, cp, cp, cp, sz, sz, vp, vp, vp]
        L.blsgpu_aggregate_priv_keys_secure_dev.argtypes = [vp, vp, vp, vp, sz, sz, vp, vp, vp, vp]
        L.blsgpu_timing_enable.argtypes = [vp, ctypes.c_int]
        L.blsgpu_timing_read.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int), sz,
                                         ctypes.POINTER(sz)]
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
        self._check(self.lib.blsgpu_ctx_set_mp_threshold(self.h, pairs), "blsgpu_ctx_set_mp_threshold")

    def mad_probe(self, target_ms=30.0, stream=None):
        """the chip's v_mad_i64_i32 rate right now, in 10^12 multiply-adds per second (a probe kernel of ~target_ms)"""
        out = ctypes.c_double(0.0)
        self._check(self.lib.blsgpu_timing_mad_probe(self.h, float(target_ms), ctypes.byref(out), stream), "blsgpu_timing_mad_probe")
        return out.value

    def mark(self, tag=0, stream=None):
        """one dispatch of an empty kernel: brackets a timed region in a profile of the run"""
        self._check(self.lib.blsgpu_timing_mark(self.h, tag, stream), "blsgpu_timing_mark")

    def set_miller_wide_max(self, pairs):
        """Calls of at most `pairs` pairs run the wide Miller loop (one pair per two-wavefront workgroup); 0: never."""
        self._check(self.lib.blsgpu_ctx_set_miller_wide_max(self.h, pairs), "blsgpu_ctx_set_miller_wide_max")

    def set_mp3_threshold(self, pairs):
        """Throughput kernel: three pairs per wavefront from `pairs` pairs per call on, two below."""
        self._check(self.lib.blsgpu_ctx_set_mp3_threshold(self.h, pairs), "blsgpu_ctx_set_mp3_threshold")

    def set_ls_threshold(self, pairs, min_group=64):
        """Calls >= pairs with groups >= min_group use the line-stream kernels; pairs = None: never."""
        self._check(self.lib.blsgpu_ctx_set_ls_threshold(self.h, (1 << 64) - 1 if pairs is None else pairs, min_group),
                    "blsgpu_ctx_set_ls_threshold")

    WS_FIELDS = ("partials", "staging", "lines", "line_products", "flags_and_lists", "group_sums", "slots", "total")

    def workspace_bytes(self):
        """bytes of HBM the context's grow-only workspace holds, by purpose (include/blsgpu.h BLSGPU_WS_*)"""
        out = (ctypes.c_size_t * len(self.WS_FIELDS))()
        self._check(self.lib.blsgpu_ctx_workspace_bytes(self.h, out), "blsgpu_ctx_workspace_bytes")
        return dict(zip(self.WS_FIELDS, (int(v) for v in out)))

    def verify_pipeline(self, neg_g1, sig, hashes, n, keys_affine=None, key_pts=None, key_scalars=None, k=0):
        """blsgpu_verify_pipeline: e(-G1, sig) * prod e(P_i, H(m_i)) -- hash to G2, key sums and multi-pairing in one
        call on host buffers (ctypes only: no torch)"""
        out = ctypes.create_string_buffer(576)
        self._check(self.lib.blsgpu_verify_pipeline(self.h, neg_g1, sig, hashes if n else None, n, keys_affine, key_pts, key_scalars,
                                                    k, out), "blsgpu_verify_pipeline")
        return out.raw

    def set_ls_teams(self, teams):
        self._check(self.lib.blsgpu_ctx_set_ls_teams(self.h, teams), "blsgpu_ctx_set_ls_teams")

    def set_fexp_team_threshold(self, results):
        """calls with >= results final exponentiations run them six lanes each; None: never"""
        self._check(self.lib.blsgpu_ctx_set_fexp_team_threshold(self.h, (1 << 64) - 1 if results is None else results),
                    "blsgpu_ctx_set_fexp_team_threshold")

    def set_bulk_event(self, event_handle):
        """hipEvent_t handle (int; torch: event.cuda_event after a first record) recorded after the chip-filling
        kernels of every Miller stage, or None"""
        self._check(self.lib.blsgpu_ctx_set_bulk_event(self.h, event_handle), "blsgpu_ctx_set_bulk_event")

    def reserve(self, max_pairs):
        self._check(self.lib.blsgpu_ctx_reserve(self.h, max_pairs), "blsgpu_ctx_reserve")

    def trim(self):
        self._check(self.lib.blsgpu_ctx_trim(self.h), "blsgpu_ctx_trim")

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
        self._check(self.lib.blsgpu_pairing_multi(self.h, g1, g2, self._inf(inf, n), n, out), "blsgpu_pairing_multi")
        return out.raw

    def miller_loop_batch(self, g1: bytes, g2: bytes, n: int, inf=None) -> bytes:
        """n x 576 bytes: the reference's fq_miller_loop value of every pair."""
        if len(g1) != 96 * n or len(g2) != 192 * n:
            raise ValueError("g1/g2 length does not match n")
        out = ctypes.create_string_buffer(max(1, 576 * n))
        self._check(self.lib.blsgpu_miller_loop_batch(self.h, g1, g2, self._inf(inf, n), n, out), "blsgpu_miller_loop_batch")
        return out.raw[:576 * n]

    def line_eval_batch(self, r: bytes, q, p: bytes, n: int) -> bytes:
        """fq2_double_line_eval(R, P) (q None) / fq2_add_line_eval(R, Q, P) for n triples -> n x 576 bytes."""
        if len(r) != 192 * n or len(p) != 96 * n or (q is not None and len(q) != 192 * n):
            raise ValueError("buffer lengths do not match n")
        out = ctypes.create_string_buffer(max(1, 576 * n))
        self._check(self.lib.blsgpu_line_eval_batch(self.h, r, q, p, n, out), "blsgpu_line_eval_batch")
        return out.raw[:576 * n]

    def final_exp(self, x: bytes) -> bytes:
        if len(x) != 576:
            raise ValueError("Fq12 must be 576 bytes")
        out = ctypes.create_string_buffer(576)
        self._check(self.lib.blsgpu_final_exp(self.h, x, out), "blsgpu_final_exp")
        return out.raw

    def final_exp_batch(self, xs: bytes) -> bytes:
        if len(xs) % 576:
            raise ValueError("need m x 576 bytes")
        out = ctypes.create_string_buffer(max(1, len(xs)))
        self._check(self.lib.blsgpu_final_exp_batch(self.h, xs, len(xs) // 576, out), "blsgpu_final_exp_batch")
        return out.raw[:len(xs)]

    FQ12_OPS = {"add": 0, "sub": 1, "mul": 2, "neg": 3, "inv": 4}

    def fq12_op(self, op: str, a: bytes, b: bytes = None) -> bytes:
        """fq12_add / sub / mul / neg / invert on n elements (n x 576 bytes each)."""
        if len(a) % 576 or (b is not None and len(b) != len(a)):
            raise ValueError("need n x 576 bytes")
        out = ctypes.create_string_buffer(max(1, len(a)))
        self._check(self.lib.blsgpu_fq12_op_batch(self.h, self.FQ12_OPS[op], a, b, len(a) // 576, out), "blsgpu_fq12_op_batch")
        return out.raw[:len(a)]

    def fq12_pow(self, a: bytes, e: int) -> bytes:
        if len(a) % 576 or e < 0:
            raise ValueError("need n x 576 bytes and a non-negative exponent")
        eb = e.to_bytes(max(1, (e.bit_length() + 7) // 8), "big")
        out = ctypes.create_string_buffer(max(1, len(a)))
        self._check(self.lib.blsgpu_fq12_pow_batch(self.h, a, eb, len(eb), len(a) // 576, out), "blsgpu_fq12_pow_batch")
        return out.raw[:len(a)]

    def pairing_multi_batch(self, g1: bytes, g2: bytes, gsz: int, groups: int, inf=None) -> bytes:
        n = gsz * groups
        if len(g1) != 96 * n or len(g2) != 192 * n:
            raise ValueError("g1/g2 length does not match gsz * groups")
        out = ctypes.create_string_buffer(max(1, 576 * groups))
        self._check(self.lib.blsgpu_pairing_multi_batch(self.h, g1, g2, self._inf(inf, n), gsz, groups, out), "blsgpu_pairing_multi_batch")
        return out.raw[:576 * groups]

    def _decompress(self, fn, name, insz, data):
        if len(data) % insz:
            raise ValueError("need n x %d bytes" % insz)
        k = len(data) // insz
        out = ctypes.create_string_buffer(max(1, 2 * len(data)))
        ok = ctypes.create_string_buffer(max(1, k))
        self._check(fn(self.h, data, k, out, ok), name)
        return out.raw[:2 * len(data)], [b != 0 for b in ok.raw[:k]]

    def g1_decompress(self, data: bytes):
        """n x 48 bytes -> (n x 96 bytes affine, [accepted])."""
        return self._decompress(self.lib.blsgpu_g1_decompress, "blsgpu_g1_decompress", 48, data)

    def g2_decompress(self, data: bytes):
        """n x 96 bytes -> (n x 192 bytes affine, [accepted])."""
        return self._decompress(self.lib.blsgpu_g2_decompress, "blsgpu_g2_decompress", 96, data)

    def hash_to_g2(self, msg_hashes: bytes) -> bytes:
        """n x 32-byte message hashes -> n x 192 bytes affine G2 (SHA-256 chain on the GPU too)."""
        if len(msg_hashes) % 32:
            raise ValueError("need n x 32 bytes")
        out = ctypes.create_string_buffer(max(1, 6 * len(msg_hashes)))
        self._check(self.lib.blsgpu_hash_to_g2(self.h, msg_hashes, len(msg_hashes) // 32, out), "blsgpu_hash_to_g2")
        return out.raw[:6 * len(msg_hashes)]

    def map_to_g2(self, t: bytes) -> bytes:
        """t: n x 192 bytes (t0.c0, t0.c1, t1.c0, t1.c1) -> n x 192 bytes affine G2."""
        if len(t) % 192:
            raise ValueError("need n x 192 bytes")
        out = ctypes.create_string_buffer(max(1, len(t)))
        self._check(self.lib.blsgpu_map_to_g2(self.h, t, len(t) // 192, out), "blsgpu_map_to_g2")
        return out.raw[:len(t)]

    def _msm(self, fn, psz, pts, scalars, k, groups):
        n = k * groups
        if len(pts) != psz * n:
            raise ValueError("point buffer length does not match k * groups")
        sb = None
        if scalars is not None:
            sb = scalars if isinstance(scalars, (bytes, bytearray)) else b"".join(int(s).to_bytes(32, "big") for s in scalars)
            if len(sb) != 32 * n:
                raise ValueError("scalar buffer length does not match k * groups")
            sb = bytes(sb)
        out = ctypes.create_string_buffer(psz * groups)
        inf = ctypes.create_string_buffer(max(1, groups))
        self._check(fn(self.h, bytes(pts), sb, k, groups, out, inf), fn.__name__)
        return out.raw, [bool(b) for b in inf.raw[:groups]]

    def g1_msm(self, pts, scalars, k, groups=1):
        """-> (groups x 96 affine bytes, [is_infinity])"""
        return self._msm(self.lib.blsgpu_g1_msm, 96, pts, scalars, k, groups)

    def g2_msm(self, pts, scalars, k, groups=1):
        return self._msm(self.lib.blsgpu_g2_msm, 192, pts, scalars, k, groups)

    def g1_mul_gen(self, scalars, add=None, n_add=0, aff=True, ser=True):
        """(s_i mod n) G1 (+ A) for n scalars (n x 32 bytes big-endian, or ints below 2^256) on the fixed-base table;
        add: None, one point (n_add = 1) or n points (n_add = n), 96 bytes affine each.
        -> (n x 96 affine bytes or None, n x 48 serialised bytes or None)"""
        sb = scalars if isinstance(scalars, (bytes, bytearray)) else b"".join(int(s).to_bytes(32, "big") for s in scalars)
        if len(sb) % 32:
            raise ValueError("need n x 32 scalar bytes")
        n = len(sb) // 32
        if n_add not in (0, 1, n) or len(add or b"") != 96 * n_add:
            raise ValueError("add must hold 0, 1 or n points of 96 bytes")
        if not (aff or ser):
            raise ValueError("ask for at least one output")
        oa = ctypes.create_string_buffer(max(1, 96 * n)) if aff else None
        os_ = ctypes.create_string_buffer(max(1, 48 * n)) if ser else None
        self._check(self.lib.blsgpu_g1_mul_gen(self.h, bytes(sb), n, bytes(add) if n_add else None, n_add, oa, os_), "blsgpu_g1_mul_gen")
        return (oa.raw[:96 * n] if aff else None), (os_.raw[:48 * n] if ser else None)

    def g1_mul_gen_secret(self, scalars, aff=True, ser=True):
        """s_i G1 for n SECRET scalars (n x 32 bytes big-endian, or ints below 2^256) on the scalar-independent schedule of
        blsgpu_g1_mul_gen_secret; the bytes of g1_mul_gen.
        -> (n x 96 affine bytes or None, n x 48 serialised bytes or None)"""
        sb = scalars if isinstance(scalars, (bytes, bytearray)) else b"".join(int(s).to_bytes(32, "big") for s in scalars)
        if len(sb) % 32:
            raise ValueError("need n x 32 scalar bytes")
        n = len(sb) // 32
        if not (aff or ser):
            raise ValueError("ask for at least one output")
        oa = ctypes.create_string_buffer(max(1, 96 * n)) if aff else None
        os_ = ctypes.create_string_buffer(max(1, 48 * n)) if ser else None
        self._check(self.lib.blsgpu_g1_mul_gen_secret(self.h, bytes(sb), n, oa, os_), "blsgpu_g1_mul_gen_secret")
        return (oa.raw[:96 * n] if aff else None), (os_.raw[:48 * n] if ser else None)

    def g1_mul_gen_secret_dev(self, d_scalars, n, d_out_aff, d_out_ser, stream=0):
        self._check(self.lib.blsgpu_g1_mul_gen_secret_dev(self.h, d_scalars, n, d_out_aff, d_out_ser, stream),
                    "blsgpu_g1_mul_gen_secret_dev")

    def hd_children(self, chain_code, parent_pk_aff, parent_sk, indices, aff=True, ser=True):
        """HD children of one parent (blsgpu_hd_children): parent_sk None = public derivation.
        -> (n x 32 chain codes, n x 32 child keys or None, n x 96 affine keys or None, n x 48 serialised keys or None)"""
        if len(chain_code) != 32 or len(parent_pk_aff) != 96 or (parent_sk is not None and len(parent_sk) != 32):
            raise ValueError("chain code 32, parent key 96 (and private key 32) bytes")
        n = len(indices)
        if any(i < 0 or i >= 1 << 32 for i in indices):
            raise OverflowError("child indices are 32-bit")           # (a c_uint32 array would wrap them silently)
        idx = (ctypes.c_uint32 * max(1, n))(*indices)
        chain = ctypes.create_string_buffer(max(1, 32 * n))
        sk = ctypes.create_string_buffer(max(1, 32 * n)) if parent_sk is not None else None
        oa = ctypes.create_string_buffer(max(1, 96 * n)) if aff else None
        os_ = ctypes.create_string_buffer(max(1, 48 * n)) if ser else None
        self._check(self.lib.blsgpu_hd_children(self.h, bytes(chain_code), bytes(parent_pk_aff),
                                                None if parent_sk is None else bytes(parent_sk), idx, n, chain, sk, oa, os_),
                    "blsgpu_hd_children")
        return (chain.raw[:32 * n], sk.raw[:32 * n] if sk is not None else None, oa.raw[:96 * n] if aff else None,
                os_.raw[:48 * n] if ser else None)

    def g1_mul_gen_dev(self, d_scalars, n, d_out_aff, d_out_ser, stream=0, d_add=None, n_add=0):
        self._check(self.lib.blsgpu_g1_mul_gen_dev(self.h, d_scalars, n, d_add, n_add, d_out_aff, d_out_ser, stream),
                    "blsgpu_g1_mul_gen_dev")

    def hd_children_dev(self, chain_code, parent_pk_aff, parent_sk, d_indices, n, d_out_chain, d_out_sk, d_out_pk_aff,
                        d_out_pk_ser, stream=0):
        self._check(self.lib.blsgpu_hd_children_dev(self.h, bytes(chain_code), bytes(parent_pk_aff),
                                                    None if parent_sk is None else bytes(parent_sk), d_indices, n, d_out_chain,
                                                    d_out_sk, d_out_pk_aff, d_out_pk_ser, stream), "blsgpu_hd_children_dev")

    def hd_paths_secret(self, parents, parent_of, paths, aff=True, ser=True, fp=True):
        """hd_paths in private mode on the scalar-independent schedule (blsgpu_hd_paths_secret): the same arguments without
        `priv`, the same outputs."""
        return self.hd_paths(parents, True, parent_of, paths, aff, ser, fp, secret=True)

    def hd_paths_secret_dev(self, d_parents, n_parents, d_parent_of, d_indices, depth, n, d_out_chain, d_out_sk, d_out_pk_aff,
                            d_out_pk_ser, d_out_parent_fp, stream=0):
        self._check(self.lib.blsgpu_hd_paths_secret_dev(self.h, d_parents, n_parents, d_parent_of, d_indices, depth, n, d_out_chain,
                                                        d_out_sk, d_out_pk_aff, d_out_pk_ser, d_out_parent_fp, stream),
                    "blsgpu_hd_paths_secret_dev")

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
        # (array("I") raises OverflowError outside 32 bits, where a c_uint32 array would wrap silently)
        flat = array.array("I", [i for p in paths for i in p] or [0])
        idx = (ctypes.c_uint32 * len(flat)).from_buffer(flat)
        pof = None
        if parent_of is not None:
            pof_arr = array.array("I", list(parent_of) or [0])
            pof = (ctypes.c_uint32 * len(pof_arr)).from_buffer(pof_arr)
        chain = ctypes.create_string_buffer(max(1, 32 * n))
        sk = ctypes.create_string_buffer(max(1, 32 * n)) if priv else None
        oa = ctypes.create_string_buffer(max(1, 96 * n)) if aff else None
        os_ = ctypes.create_string_buffer(max(1, 48 * n)) if ser else None
        of = ctypes.create_string_buffer(max(1, 4 * n)) if fp else None
        if secret:
            self._check(self.lib.blsgpu_hd_paths_secret(self.h, bytes(parents), len(parents) // HD_PARENT_BYTES, pof, idx, depth, n,
                                                        chain, sk, oa, os_, of), "blsgpu_hd_paths_secret")
        else:
            self._check(self.lib.blsgpu_hd_paths(self.h, bytes(parents), len(parents) // HD_PARENT_BYTES, 1 if priv else 0, pof, idx, depth, n,
                                                 chain, sk, oa, os_, of), "blsgpu_hd_paths")
        return (chain.raw[:32 * n], sk.raw[:32 * n] if priv else None, oa.raw[:96 * n] if aff else None,
                os_.raw[:48 * n] if ser else None, of.raw[:4 * n] if fp else None)

    def hd_paths_dev(self, d_parents, n_parents, priv, d_parent_of, d_indices, depth, n, d_out_chain, d_out_sk, d_out_pk_aff,
                     d_out_pk_ser, d_out_parent_fp, stream=0):
        self._check(self.lib.blsgpu_hd_paths_dev(self.h, d_parents, n_parents, 1 if priv else 0, d_parent_of, d_indices, depth, n,
                                                 d_out_chain, d_out_sk, d_out_pk_aff, d_out_pk_ser, d_out_parent_fp, stream),
                    "blsgpu_hd_paths_dev")

    def g1_poly_check_secret(self, commit, n_polys, t, poly, x, s, aff=False):
        """g1_poly_check for SECRET fragments s on the scalar-independent schedule of blsgpu_g1_poly_check_secret: the same
        arguments (s is required: there is no evaluation-only mode), the same bytes.
        -> (n status bytes (1 equal, 0 not, 2 undecided), n x 96 affine Horner values or None)"""
        if s is None:
            raise ValueError("the secret form has no evaluation-only mode")
        return self.g1_poly_check(commit, n_polys, t, poly, x, s, aff, secret=True)

    def g1_poly_check_secret_dev(self, d_commit, n_polys, t, d_poly, d_x, d_s, n, d_status, d_out_aff, stream=0):
        self._check(self.lib.blsgpu_g1_poly_check_secret_dev(self.h, d_commit, n_polys, t, d_poly, d_x, d_s, n, d_status, d_out_aff,
                                                             stream), "blsgpu_g1_poly_check_secret_dev")

    def g1_poly_check(self, commit, n_polys, t, poly, x, s=None, aff=False, secret=False):
        """Feldman share checks (blsgpu_g1_poly_check): commit n_polys x t x 96 affine bytes, poly n indices, x / s n x 32
        bytes big-endian (or ints below 2^256); s None = evaluation only.
        -> (n status bytes (1 equal, 0 not, 2 undecided) or None, n x 96 affine Horner values or None)"""
        def as_bytes(v):
            return v if isinstance(v, (bytes, bytearray)) else b"".join(int(a).to_bytes(32, "big") for a in v)
        xb = as_bytes(x)
        n = len(poly)
        sb = as_bytes(s) if s is not None else None
        if len(xb) != 32 * n or (sb is not None and len(sb) != 32 * n) or len(commit) != 96 * n_polys * t:
            raise ValueError("need n x 32 bytes of x (and s) and n_polys x t x 96 bytes of commitments")
        if sb is None and not aff:
            raise ValueError("ask for at least one output")
        if any(p < 0 or p >= 1 << 32 for p in poly):
            raise OverflowError("polynomial indices are 32-bit")
        idx = (ctypes.c_uint32 * max(1, n))(*poly)
        st = ctypes.create_string_buffer(max(1, n)) if sb is not None else None
        oa = ctypes.create_string_buffer(max(1, 96 * n)) if aff else None
        name = "blsgpu_g1_poly_check_secret" if secret else "blsgpu_g1_poly_check"
        self._check(getattr(self.lib, name)(self.h, bytes(commit), n_polys, t, idx, bytes(xb), None if sb is None else bytes(sb), n,
                                            st, oa), name)
        return (st.raw[:n] if st is not None else None), (oa.raw[:96 * n] if aff else None)

    def g1_poly_check_dev(self, d_commit, n_polys, t, d_poly, d_x, d_s, n, d_status, d_out_aff, stream=0):
        self._check(self.lib.blsgpu_g1_poly_check_dev(self.h, d_commit, n_polys, t, d_poly, d_x, d_s, n, d_status, d_out_aff, stream),
                    "blsgpu_g1_poly_check_dev")

    def _subgroup(self, g, psz, pts):
        if len(pts) % psz:
            raise ValueError("need n x %d bytes" % psz)
        n = len(pts) // psz
        st = ctypes.create_string_buffer(max(1, n))
        name = "blsgpu_%s_subgroup_check" % g
        self._check(getattr(self.lib, name)(self.h, bytes(pts), n, st), name)
        return st.raw[:n]

    def g1_subgroup(self, pts):
        """n x 96 affine bytes ((0, 0) = infinity) -> n status bytes: 1 in G1, 2 on the curve outside it, 0 off the curve"""
        return self._subgroup("g1", 96, pts)

    def g2_subgroup(self, pts):
        """n x 192 affine bytes (all zero = infinity) -> n status bytes: 1 in G2, 2 on the twist outside it, 0 off it"""
        return self._subgroup("g2", 192, pts)

    def g1_subgroup_dev(self, d_pts, n, d_status, stream=0):
        self._check(self.lib.blsgpu_g1_subgroup_check_dev(self.h, d_pts, n, d_status, stream), "blsgpu_g1_subgroup_check_dev")

    def g2_subgroup_dev(self, d_pts, n, d_status, stream=0):
        self._check(self.lib.blsgpu_g2_subgroup_check_dev(self.h, d_pts, n, d_status, stream), "blsgpu_g2_subgroup_check_dev")

    @staticmethod
    def _scalars(v, n, what):
        """n x 32 bytes big-endian from bytes or from ints below 2^256"""
        b = bytes(v) if isinstance(v, (bytes, bytearray)) else b"".join(int(a).to_bytes(32, "big") for a in v)
        if len(b) != 32 * n:
            raise ValueError("%s must hold k * groups values of 32 bytes" % what)
        return b

    def lagrange_at_zero(self, x, k, groups=1):
        """Lagrange coefficients at zero of `groups` groups of k evaluation points (blsgpu_lagrange_at_zero): x
        groups x k x 32 bytes big-endian (or ints below 2^256), 1 <= k <= LAGRANGE_MAX_K.
        -> (groups x k x 32 coefficient bytes, groups status bytes: 1 written, 0 where the reference asserts -- zeros)"""
        n = k * groups
        co = ctypes.create_string_buffer(max(1, 32 * n))
        st = ctypes.create_string_buffer(max(1, groups))
        self._check(self.lib.blsgpu_lagrange_at_zero(self.h, self._scalars(x, n, "x"), k, groups, co, st), "blsgpu_lagrange_at_zero")
        return co.raw[:32 * n], st.raw[:groups]

    def fr_interpolate_at_zero(self, x, y, k, groups=1):
        """sum_j L_j y_j mod n per group (blsgpu_fr_interpolate_at_zero): x, y groups x k x 32 bytes big-endian (or ints
        below 2^256).  -> (groups x 32 bytes, groups status bytes)"""
        n = k * groups
        out = ctypes.create_string_buffer(max(1, 32 * groups))
        st = ctypes.create_string_buffer(max(1, groups))
        self._check(self.lib.blsgpu_fr_interpolate_at_zero(self.h, self._scalars(x, n, "x"), self._scalars(y, n, "y"), k, groups, out, st),
                    "blsgpu_fr_interpolate_at_zero")
        return out.raw[:32 * groups], st.raw[:groups]

    def threshold_combine(self, sigs, x, k, groups=1):
        """sum_j L_j sig_j per group (blsgpu_threshold_combine): sigs groups x k x 192 affine bytes, x as above.
        -> (groups x 192 affine bytes, [is_infinity], groups status bytes)"""
        n = k * groups
        if len(sigs) != 192 * n:
            raise ValueError("signature buffer length does not match k * groups")
        out = ctypes.create_string_buffer(max(1, 192 * groups))
        inf = ctypes.create_string_buffer(max(1, groups))
        st = ctypes.create_string_buffer(max(1, groups))
        self._check(self.lib.blsgpu_threshold_combine(self.h, bytes(sigs), self._scalars(x, n, "x"), k, groups, out, inf, st),
                    "blsgpu_threshold_combine")
        return out.raw[:192 * groups], [bool(b) for b in inf.raw[:groups]], st.raw[:groups]

    def lagrange_at_zero_dev(self, d_x, k, groups, d_out_coeffs, d_status, stream=0):
        self._check(self.lib.blsgpu_lagrange_at_zero_dev(self.h, d_x, k, groups, d_out_coeffs, d_status, stream), "blsgpu_lagrange_at_zero_dev")

    def fr_interpolate_at_zero_dev(self, d_x, d_y, k, groups, d_out, d_status, stream=0):
        self._check(self.lib.blsgpu_fr_interpolate_at_zero_dev(self.h, d_x, d_y, k, groups, d_out, d_status, stream),
                    "blsgpu_fr_interpolate_at_zero_dev")

    def threshold_combine_dev(self, d_sigs, d_x, k, groups, d_out, d_out_inf, d_status, stream=0):
        self._check(self.lib.blsgpu_threshold_combine_dev(self.h, d_sigs, d_x, k, groups, d_out, d_out_inf, d_status, stream),
                    "blsgpu_threshold_combine_dev")

    def sig_shares_check(self, sigs, keys, key_idx, x, msg_hashes, weights, k, groups=1, scaled=True):
        """Signature shares of `groups` sessions of k shares checked on the device (blsgpu_sig_shares_check): sigs groups x k x
        192 affine bytes, keys n_keys x 96 affine bytes, key_idx groups x k indices into them, x groups x k x 32 bytes
        big-endian (or ints below 2^256; None when not scaled), msg_hashes groups x 32 bytes, weights groups x k x 8 bytes
        big-endian (or ints below 2^64; a zero weight is taken as 1).
        -> (groups x k status bytes: 1 valid, 0 invalid, 2 not decided (the key is off the curve or outside G1); groups session
        status bytes: 0 where the player set is refused; (rounds, node tests))"""
        n = k * groups
        wb = bytes(weights) if isinstance(weights, (bytes, bytearray)) else b"".join(int(w).to_bytes(8, "big") for w in weights)
        if len(sigs) != 192 * n or len(keys) % 96 or len(key_idx) != n or len(msg_hashes) != 32 * groups or len(wb) != 8 * n:
            raise ValueError("buffer lengths do not match k * groups")
        if scaled and x is None:
            raise ValueError("scaled shares need the player numbers")
        if any(i < 0 or i >= 1 << 32 for i in key_idx):
            raise OverflowError("key indices are 32-bit")
        idx = (ctypes.c_uint32 * max(1, n))(*key_idx)
        st = ctypes.create_string_buffer(max(1, n))
        ss = ctypes.create_string_buffer(max(1, groups))
        stats = (ctypes.c_uint64 * 2)()
        self._check(self.lib.blsgpu_sig_shares_check(self.h, bytes(sigs), bytes(keys), len(keys) // 96, idx,
                                                     self._scalars(x, n, "x") if scaled else None, bytes(msg_hashes), wb,
                                                     1 if scaled else 0, k, groups, st, ss, stats), "blsgpu_sig_shares_check")
        return st.raw[:n], ss.raw[:groups], (int(stats[0]), int(stats[1]))

    def sig_shares_check_dev(self, d_sigs, d_keys, n_keys, d_key_idx, d_x, d_msg_hashes, d_weights, scaled, k, groups, d_status,
                             d_session_status, stream=0):
        """-> (rounds, node tests); the status bytes are in d_status / d_session_status when the call returns"""
        stats = (ctypes.c_uint64 * 2)()
        self._check(self.lib.blsgpu_sig_shares_check_dev(self.h, d_sigs, d_keys, n_keys, d_key_idx, d_x, d_msg_hashes, d_weights,
                                                         1 if scaled else 0, k, groups, d_status, d_session_status, stats, stream),
                    "blsgpu_sig_shares_check_dev")
        return int(stats[0]), int(stats[1])

    def g2_mul_secret(self, pts, scalars, aff=True, ser=True):
        """s_i P_i (or s_i P for ONE point of 192 bytes) for n scalars (n x 32 bytes big-endian, or ints below 2^256, taken as
        they are) on the scalar-independent schedule of blsgpu_g2_mul_secret.
        -> (n x 192 affine bytes or None, n x 96 serialised bytes or None, [is_infinity])"""
        sb = scalars if isinstance(scalars, (bytes, bytearray)) else b"".join(int(s).to_bytes(32, "big") for s in scalars)
        if len(sb) % 32 or len(pts) % 192:
            raise ValueError("need n x 32 scalar bytes and points of 192 bytes")
        n, n_pts = len(sb) // 32, len(pts) // 192
        if not (aff or ser):
            raise ValueError("ask for at least one output")
        oa = ctypes.create_string_buffer(max(1, 192 * n)) if aff else None
        os_ = ctypes.create_string_buffer(max(1, 96 * n)) if ser else None
        inf = ctypes.create_string_buffer(max(1, n))
        self._check(self.lib.blsgpu_g2_mul_secret(self.h, bytes(pts), n_pts, bytes(sb), n, oa, os_, inf), "blsgpu_g2_mul_secret")
        return (oa.raw[:192 * n] if aff else None), (os_.raw[:96 * n] if ser else None), [bool(b) for b in inf.raw[:n]]

    def sign(self, sks, msg_hashes, aff=True, ser=True):
        """sk_i H(h_i) (or sk_i H(h) for ONE hash of 32 bytes) for n private keys (n x 32 bytes big-endian, or ints): the hash
        to G2 and the scalar-independent multiplication in one call (blsgpu_sign).
        -> (n x 192 affine bytes or None, n x 96 bytes of Signature.serialize() or None)"""
        sb = sks if isinstance(sks, (bytes, bytearray)) else b"".join(int(s).to_bytes(32, "big") for s in sks)
        if len(sb) % 32 or len(msg_hashes) % 32:
            raise ValueError("need n x 32 key bytes and hashes of 32 bytes")
        n, n_msg = len(sb) // 32, len(msg_hashes) // 32
        if not (aff or ser):
            raise ValueError("ask for at least one output")
        oa = ctypes.create_string_buffer(max(1, 192 * n)) if aff else None
        os_ = ctypes.create_string_buffer(max(1, 96 * n)) if ser else None
        self._check(self.lib.blsgpu_sign(self.h, bytes(sb), bytes(msg_hashes), n_msg, n, oa, os_), "blsgpu_sign")
        return (oa.raw[:192 * n] if aff else None), (os_.raw[:96 * n] if ser else None)

    def g2_mul_secret_dev(self, d_pts, n_pts, d_scalars, n, d_out_aff, d_out_ser, d_out_inf=None, stream=0):
        self._check(self.lib.blsgpu_g2_mul_secret_dev(self.h, d_pts, n_pts, d_scalars, n, d_out_aff, d_out_ser, d_out_inf, stream),
                    "blsgpu_g2_mul_secret_dev")

    def sign_dev(self, d_sks, d_msg_hashes, n_msg, n, d_out_aff, d_out_ser, stream=0):
        self._check(self.lib.blsgpu_sign_dev(self.h, d_sks, d_msg_hashes, n_msg, n, d_out_aff, d_out_ser, stream), "blsgpu_sign_dev")

    def threshold_deal_secret(self, coeffs, t, x, commit=True, frag=True):
        """Commitments and fragments of len(coeffs) / t polynomials with SECRET coefficients (blsgpu_threshold_deal_secret):
        coeffs n_polys x t x 32 bytes big-endian (or ints below 2^256), x the n_x points the fragments are taken at, likewise
        (ignored without frag).
        -> (n_polys x t x 96 affine bytes c_k G1 or None, n_polys x n_x x 32 bytes P_p(x_j) mod n or None)"""
        cb = coeffs if isinstance(coeffs, (bytes, bytearray)) else b"".join(int(c).to_bytes(32, "big") for c in coeffs)
        xb = b"" if not frag else x if isinstance(x, (bytes, bytearray)) else b"".join(int(v).to_bytes(32, "big") for v in x)
        if t < 1 or len(cb) % (32 * t) or len(xb) % 32:
            raise ValueError("need n_polys x t x 32 coefficient bytes and n_x x 32 bytes of points")
        if not (commit or frag):
            raise ValueError("ask for at least one output")
        n_polys, n_x = len(cb) // (32 * t), len(xb) // 32
        oc = ctypes.create_string_buffer(max(1, 96 * n_polys * t)) if commit else None
        of = ctypes.create_string_buffer(max(1, 32 * n_polys * n_x)) if frag else None
        self._check(self.lib.blsgpu_threshold_deal_secret(self.h, bytes(cb), n_polys, t, bytes(xb) if frag else None, n_x, oc, of),
                    "blsgpu_threshold_deal_secret")
        return (oc.raw[:96 * n_polys * t] if commit else None), (of.raw[:32 * n_polys * n_x] if frag else None)

    def threshold_deal_secret_dev(self, d_coeffs, n_polys, t, d_x, n_x, d_out_commit_aff, d_out_frag, stream=0):
        self._check(self.lib.blsgpu_threshold_deal_secret_dev(self.h, d_coeffs, n_polys, t, d_x, n_x, d_out_commit_aff, d_out_frag, stream),
                    "blsgpu_threshold_deal_secret_dev")

    def fr_interpolate_at_zero_secret(self, x, y, k, groups=1):
        """fr_interpolate_at_zero for SECRET y (shares) on the masked sums of blsgpu_fr_interpolate_at_zero_secret: the same
        arguments, the same bytes.  -> (groups x 32 bytes, groups status bytes)"""
        n = k * groups
        out = ctypes.create_string_buffer(max(1, 32 * groups))
        st = ctypes.create_string_buffer(max(1, groups))
        self._check(self.lib.blsgpu_fr_interpolate_at_zero_secret(self.h, self._scalars(x, n, "x"), self._scalars(y, n, "y"), k, groups,
                                                                  out, st), "blsgpu_fr_interpolate_at_zero_secret")
        return out.raw[:32 * groups], st.raw[:groups]

    def fr_interpolate_at_zero_secret_dev(self, d_x, d_y, k, groups, d_out, d_status, stream=0):
        self._check(self.lib.blsgpu_fr_interpolate_at_zero_secret_dev(self.h, d_x, d_y, k, groups, d_out, d_status, stream),
                    "blsgpu_fr_interpolate_at_zero_secret_dev")

    def fr_sum_secret(self, y, k, groups=1, pk=False, aff=False, ser=False):
        """sum_j y_j mod n per group for SECRET y (blsgpu_fr_sum_secret: a player's share from the fragments it was dealt): y
        groups x k x 32 bytes big-endian (or ints below 2^256), k >= 1.  pk: both forms of the public key of every sum
        (aff / ser: one of them), multiplied on the device by k_fix_mul_secret.
        -> (groups x 32 bytes, groups x 96 affine bytes or None, groups x 48 serialised bytes or None)"""
        if k < 1:
            raise ValueError("k must be at least 1")
        aff, ser = aff or pk, ser or pk
        out = ctypes.create_string_buffer(max(1, 32 * groups))
        oa = ctypes.create_string_buffer(max(1, 96 * groups)) if aff else None
        os_ = ctypes.create_string_buffer(max(1, 48 * groups)) if ser else None
        self._check(self.lib.blsgpu_fr_sum_secret(self.h, self._scalars(y, k * groups, "y"), k, groups, out, oa, os_), "blsgpu_fr_sum_secret")
        return out.raw[:32 * groups], (oa.raw[:96 * groups] if aff else None), (os_.raw[:48 * groups] if ser else None)

    def fr_sum_secret_dev(self, d_y, k, groups, d_out, d_out_pk_aff, d_out_pk_ser, stream=0):
        self._check(self.lib.blsgpu_fr_sum_secret_dev(self.h, d_y, k, groups, d_out, d_out_pk_aff, d_out_pk_ser, stream),
                    "blsgpu_fr_sum_secret_dev")

    def sign_threshold(self, sks, x, k, msg_hashes, groups=1, aff=True, ser=True):
        """Unit signatures (lambda_j sk_j mod n) H(h) of `groups` sessions of k signers (blsgpu_sign_threshold): sks, x
        groups x k x 32 bytes big-endian (or ints below 2^256), msg_hashes ONE hash of 32 bytes or one per session.
        -> (groups x k x 192 affine bytes or None, groups x k x 96 serialised bytes or None, [is_infinity], groups status bytes)"""
        n = k * groups
        if len(msg_hashes) % 32:
            raise ValueError("message hashes are 32 bytes")
        if not (aff or ser):
            raise ValueError("ask for at least one output")
        oa = ctypes.create_string_buffer(max(1, 192 * n)) if aff else None
        os_ = ctypes.create_string_buffer(max(1, 96 * n)) if ser else None
        inf = ctypes.create_string_buffer(max(1, n))
        st = ctypes.create_string_buffer(max(1, groups))
        self._check(self.lib.blsgpu_sign_threshold(self.h, self._scalars(sks, n, "sks"), self._scalars(x, n, "x"), k, groups, bytes(msg_hashes),
                                                   len(msg_hashes) // 32, oa, os_, inf, st), "blsgpu_sign_threshold")
        return (oa.raw[:192 * n] if aff else None), (os_.raw[:96 * n] if ser else None), [bool(b) for b in inf.raw[:n]], st.raw[:groups]

    def sign_threshold_dev(self, d_sks, d_x, k, groups, d_msg_hashes, n_msg, d_out_aff, d_out_ser, d_out_inf, d_status, stream=0):
        self._check(self.lib.blsgpu_sign_threshold_dev(self.h, d_sks, d_x, k, groups, d_msg_hashes, n_msg, d_out_aff, d_out_ser, d_out_inf,
                                                       d_status, stream), "blsgpu_sign_threshold_dev")

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
        32 bytes big-endian each.  pk_hash: see _pk_hashes.  -> exponent bytes (, groups x 32 digest bytes)"""
        pks_ser = bytes(pks_ser)
        ph = self._pk_hashes(pks_ser, k, groups, pk_hash)
        out = ctypes.create_string_buffer(max(1, 32 * m * groups))
        dg = ctypes.create_string_buffer(max(1, 32 * groups)) if want_pk_hash else None
        self._check(self.lib.blsgpu_hash_pks(self.h, None if ph else pks_ser, k, groups, ph, m, out, dg), "blsgpu_hash_pks")
        return (out.raw[:32 * m * groups], dg.raw[:32 * groups]) if want_pk_hash else out.raw[:32 * m * groups]

    def aggregate_pub_keys_secure(self, pts_aff, pks_ser, k, groups=1, pk_hash=None):
        """sum_i t_i P_i per group (blsgpu_aggregate_pub_keys_secure): pts_aff groups x k x 96 affine bytes, pks_ser the same
        keys serialised, both in the order to be hashed.  -> (groups x 96 affine bytes, [is_infinity])"""
        pks_ser = bytes(pks_ser)
        if len(pts_aff) != 96 * k * groups:
            raise ValueError("point buffer length does not match k * groups")
        ph = self._pk_hashes(pks_ser, k, groups, pk_hash)
        out = ctypes.create_string_buffer(max(1, 96 * groups))
        inf = ctypes.create_string_buffer(max(1, groups))
        self._check(self.lib.blsgpu_aggregate_pub_keys_secure(self.h, bytes(pts_aff), None if ph else pks_ser, ph, k, groups, out, inf),
                    "blsgpu_aggregate_pub_keys_secure")
        return out.raw[:96 * groups], [bool(b) for b in inf.raw[:groups]]

    def aggregate_sigs_secure(self, sigs_aff, k, pks_ser, k_pks, groups=1, pk_hash=None):
        """sum_i t_i S_i per group (blsgpu_aggregate_sigs_secure): sigs_aff groups x k x 192 affine bytes in the order the
        exponents multiply them, the k exponents hashed over k_pks serialised keys per group.
        -> (groups x 192 affine bytes, [is_infinity])"""
        pks_ser = bytes(pks_ser)
        if len(sigs_aff) != 192 * k * groups:
            raise ValueError("signature buffer length does not match k * groups")
        ph = self._pk_hashes(pks_ser, k_pks, groups, pk_hash)
        out = ctypes.create_string_buffer(max(1, 192 * groups))
        inf = ctypes.create_string_buffer(max(1, groups))
        self._check(self.lib.blsgpu_aggregate_sigs_secure(self.h, bytes(sigs_aff), k, None if ph else pks_ser, k_pks, ph, groups, out, inf),
                    "blsgpu_aggregate_sigs_secure")
        return out.raw[:192 * groups], [bool(b) for b in inf.raw[:groups]]

    def aggregate_priv_keys_secure(self, sks, pks_ser, k, groups=1, pk=False, aff=False, ser=False, pk_hash=None):
        """sum_i t_i sk_i mod n per group for SECRET keys (blsgpu_aggregate_priv_keys_secure): sks groups x k x 32 bytes
        big-endian (or ints below 2^256) in the order the exponents multiply them, pks_ser in the order to be hashed,
        1 <= k <= LAGRANGE_MAX_K.  pk: both forms of the public key of every sum (aff / ser: one of them).
        -> (groups x 32 bytes, groups x 96 affine bytes or None, groups x 48 serialised bytes or None)"""
        pks_ser = bytes(pks_ser)
        ph = self._pk_hashes(pks_ser, k, groups, pk_hash)
        aff, ser = aff or pk, ser or pk
        out = ctypes.create_string_buffer(max(1, 32 * groups))
        oa = ctypes.create_string_buffer(max(1, 96 * groups)) if aff else None
        os_ = ctypes.create_string_buffer(max(1, 48 * groups)) if ser else None
        self._check(self.lib.blsgpu_aggregate_priv_keys_secure(self.h, self._scalars(sks, k * groups, "sks"), None if ph else pks_ser, ph, k,
                                                               groups, out, oa, os_), "blsgpu_aggregate_priv_keys_secure")
        return out.raw[:32 * groups], (oa.raw[:96 * groups] if aff else None), (os_.raw[:48 * groups] if ser else None)

    def hash_pks_dev(self, d_pks_ser, k, groups, d_pk_hash_in, m, d_out_ts, d_out_pk_hash=None, stream=0):
        self._check(self.lib.blsgpu_hash_pks_dev(self.h, d_pks_ser, k, groups, d_pk_hash_in, m, d_out_ts, d_out_pk_hash, stream),
                    "blsgpu_hash_pks_dev")

    def aggregate_pub_keys_secure_dev(self, d_pts_aff, d_pks_ser, d_pk_hash_in, k, groups, d_out_aff, d_out_inf=None, stream=0):
        self._check(self.lib.blsgpu_aggregate_pub_keys_secure_dev(self.h, d_pts_aff, d_pks_ser, d_pk_hash_in, k, groups, d_out_aff, d_out_inf,
                                                                  stream), "blsgpu_aggregate_pub_keys_secure_dev")

    def aggregate_sigs_secure_dev(self, d_sigs_aff, k, d_pks_ser, k_pks, d_pk_hash_in, groups, d_out_aff, d_out_inf=None, stream=0):
        self._check(self.lib.blsgpu_aggregate_sigs_secure_dev(self.h, d_sigs_aff, k, d_pks_ser, k_pks, d_pk_hash_in, groups, d_out_aff,
                                                              d_out_inf, stream), "blsgpu_aggregate_sigs_secure_dev")

    def aggregate_priv_keys_secure_dev(self, d_sks, d_pks_ser, d_pk_hash_in, k, groups, d_out, d_out_pk_aff=None, d_out_pk_ser=None, stream=0):
        self._check(self.lib.blsgpu_aggregate_priv_keys_secure_dev(self.h, d_sks, d_pks_ser, d_pk_hash_in, k, groups, d_out, d_out_pk_aff,
                                                                   d_out_pk_ser, stream), "blsgpu_aggregate_priv_keys_secure_dev")

    def timing_enable(self, on=True):
        self._check(self.lib.blsgpu_timing_enable(self.h, int(on)), "blsgpu_timing_enable")

    def timing_read(self):
        """[(kind, ms)] for every kernel launched since the last read; kinds:
        0 k_miller, 1 k_reduce, 2 k_reduce + final exponentiation, 3 k_miller_slow (the rest: include/blsgpu.h)."""
        cap = 1024
        ms = (ctypes.c_float * cap)()
        kind = (ctypes.c_int * cap)()
        cnt = ctypes.c_size_t(0)
        self._check(self.lib.blsgpu_timing_read(self.h, ms, kind, cap, ctypes.byref(cnt)), "blsgpu_timing_read")
        return [(kind[i], ms[i]) for i in range(cnt.value)]

    # device-pointer forms (integers: tensor.data_ptr(), stream.cuda_stream)
    # (d_inf: device pointer to n x 2 flag bytes, or None)
    def pairing_multi_dev(self, d_g1, d_g2, n, d_out, stream=0, d_inf=None):
        self._check(self.lib.blsgpu_pairing_multi_dev(self.h, d_g1, d_g2, d_inf, n, d_out, stream),
                    "blsgpu_pairing_multi_dev")

    def miller_loop_batch_dev(self, d_g1, d_g2, n, d_out, stream=0, d_inf=None):
        self._check(self.lib.blsgpu_miller_loop_batch_dev(self.h, d_g1, d_g2, d_inf, n, d_out, stream),
                    "blsgpu_miller_loop_batch_dev")

    def miller_product_dev(self, d_g1, d_g2, n, d_partial, stream=0, d_inf=None):
        self._check(self.lib.blsgpu_miller_product_dev(self.h, d_g1, d_g2, d_inf, n, d_partial, stream),
                    "blsgpu_miller_product_dev")

    def final_exp_product_dev(self, d_partials, m, d_out, stream=0):
        self._check(self.lib.blsgpu_final_exp_product_dev(self.h, d_partials, m, d_out, stream),
                    "blsgpu_final_exp_product_dev")

    def pairing_multi_batch_dev(self, d_g1, d_g2, gsz, groups, d_out, stream=0, d_inf=None):
        self._check(self.lib.blsgpu_pairing_multi_batch_dev(self.h, d_g1, d_g2, d_inf, gsz, groups, d_out, stream),
                    "blsgpu_pairing_multi_batch_dev")

    def miller_product_batch_dev(self, d_g1, d_g2, gsz, groups, d_partials, stream=0, d_inf=None):
        self._check(self.lib.blsgpu_miller_product_batch_dev(self.h, d_g1, d_g2, d_inf, gsz, groups, d_partials, stream),
                    "blsgpu_miller_product_batch_dev")

    def final_exp_product_batch_dev(self, d_partials, m, groups, d_out, stream=0):
        self._check(self.lib.blsgpu_final_exp_product_batch_dev(self.h, d_partials, m, groups, d_out, stream),
                    "blsgpu_final_exp_product_batch_dev")


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
