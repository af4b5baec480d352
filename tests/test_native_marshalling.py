"""What bls_py._native.Engine hands to the C ABI, and what bls_py.backend.HipProvider hands to the engine, pinned without a
GPU: every public Engine method runs over a stub library that records its calls, and the records are compared with
tests/golden/native_marshalling.json.  `python tests/test_native_marshalling.py` rewrites that file from the code it
finds; it was written from the hand-marshalled binding, so a record that changes is a change of behaviour.

A recorded argument: integers, floats and None as they are; bytes as {"bytes": ...}; a ctypes char buffer (an output) as
{"out": length}; any other ctypes array as its element type, count and bytes; byref(...) as "byref".  Contents are hex up
to 64 bytes and length + SHA-256 above.  A recorded return value is its shape: lengths, and None where an output was not
asked for."""
import ctypes
import hashlib
import json
import os
import sys

import pytest

from conftest import GOLDEN, load_golden
from bls_py import _native, backend

RECORDS = "native_marshalling.json"
H = 0x1234                                   # the context handle every call must pass first


def _blob(b):
    return {"hex": b.hex()} if len(b) <= 64 else {"len": len(b), "sha256": hashlib.sha256(b).hexdigest()}


def _arg(a):
    if a is None or isinstance(a, (int, float)):
        return a
    if isinstance(a, bytes):                 # (not bytearray: c_char_p refuses one)
        return {"bytes": _blob(a)}
    if isinstance(a, ctypes.Array):
        if a._type_ is ctypes.c_char:
            return {"out": len(a)}
        return dict(_blob(bytes(a)), array=a._type_.__name__, n=len(a))
    if type(a).__name__ == "CArgObject":
        return "byref"
    raise TypeError("the binding passed a %s to the library" % type(a).__name__)


def _shape(r):
    if r is None or isinstance(r, (int, float, str)):
        return r
    if isinstance(r, bytes):
        return {"bytes": len(r)}
    if isinstance(r, tuple):
        return [_shape(v) for v in r]
    if isinstance(r, list):
        return {"list": len(r), "of": sorted({type(v).__name__ for v in r})}
    if isinstance(r, dict):
        return {"dict": list(r)}
    raise TypeError("unexpected return value %r" % (r,))


class StubLib:
    """every attribute is a function that records (name, arguments) and returns 0 (the two string functions: bytes)"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append([name] + [_arg(a) for a in args])
            return b"blsgpu/stub" if name in ("blsgpu_version", "blsgpu_last_error") else 0
        fn.__name__ = name
        return fn


def stub_engine():
    e = _native.Engine.__new__(_native.Engine)
    e.lib, e.h = StubLib(), H
    return e


def pat(n, seed=0):
    return bytes((seed + 7 * i) & 0xff for i in range(n))


def ints(n, seed=0):
    """n scalars below 2^256 with the top and the bottom byte in use"""
    return [((0x80 + seed + i) << 248) | (0x1111 * (i + 1) + seed) for i in range(n)]


def be(vals, width=32):
    return b"".join(v.to_bytes(width, "big") for v in vals)


CASES = []


def case(cid, method, *args, **kwargs):
    assert cid not in [c[0] for c in CASES], cid
    CASES.append((cid, method, args, kwargs))


REFUSALS = set()                             # cases the binding must refuse before it reaches the library
NO_MESSAGE = set()                           # refusals raised by the interpreter itself: the type is pinned, not the wording


def refusal(cid, method, *args, **kwargs):
    case(cid, method, *args, **kwargs)
    REFUSALS.add(cid)


# ---- context, knobs and measurement aids ----
case("version", "version")
case("close", "close")
case("set_mp_threshold", "set_mp_threshold", 4096)
case("mad_probe", "mad_probe")
case("mad_probe_stream", "mad_probe", 5, stream=77)
case("mark", "mark")
case("mark_tag", "mark", 3, 77)
case("set_miller_wide_max", "set_miller_wide_max", 1536)
case("set_mp3_threshold", "set_mp3_threshold", 9000)
case("set_ls_threshold", "set_ls_threshold", 2304)
case("set_ls_threshold_never", "set_ls_threshold", None, 32)
case("workspace_bytes", "workspace_bytes")
case("set_ls_teams", "set_ls_teams", 1000)
case("set_fexp_team_threshold", "set_fexp_team_threshold", 5120)
case("set_fexp_team_threshold_never", "set_fexp_team_threshold", None)
case("set_bulk_event", "set_bulk_event", 99)
case("set_bulk_event_none", "set_bulk_event", None)
case("reserve", "reserve", 1 << 20)
case("trim", "trim")
case("timing_enable", "timing_enable")
case("timing_enable_off", "timing_enable", False)
case("timing_read", "timing_read")

# ---- pairings and Fq12 ----
case("verify_pipeline_keys", "verify_pipeline", pat(96, 1), pat(192, 2), pat(64, 3), 2, keys_affine=pat(192, 4))
case("verify_pipeline_sums", "verify_pipeline", pat(96, 1), pat(192, 2), pat(32, 3), 1, None, pat(288, 5), pat(96, 6), 3)
case("verify_pipeline_empty", "verify_pipeline", pat(96, 1), pat(192, 2), b"", 0)
for n in (1, 3):
    case("pairing_multi_%d" % n, "pairing_multi", pat(96 * n, 1), pat(192 * n, 2), n)
    case("miller_loop_batch_%d" % n, "miller_loop_batch", pat(96 * n, 1), pat(192 * n, 2), n)
case("pairing_multi_inf", "pairing_multi", pat(192, 1), pat(384, 2), 2, inf=[0, 1, 1, 0])
case("pairing_multi_inf_bytes", "pairing_multi", pat(192, 1), pat(384, 2), 2, bytearray(b"\0\1\0\0"))
refusal("pairing_multi_len", "pairing_multi", pat(96, 1), pat(192, 2), 2)
refusal("pairing_multi_len_g2", "pairing_multi", pat(96, 1), pat(191, 2), 1)
refusal("pairing_multi_inf_len", "pairing_multi", pat(96, 1), pat(192, 2), 1, inf=[0, 1, 0])
case("miller_loop_batch_inf", "miller_loop_batch", pat(192, 1), pat(384, 2), 2, inf=[0, 1, 1, 0])
refusal("miller_loop_batch_len", "miller_loop_batch", pat(96, 1), pat(192, 2), 2)
case("line_eval_batch_double", "line_eval_batch", pat(192 * 2, 1), None, pat(96 * 2, 2), 2)
case("line_eval_batch_add", "line_eval_batch", pat(192, 1), pat(192, 3), pat(96, 2), 1)
refusal("line_eval_batch_len", "line_eval_batch", pat(192, 1), pat(191, 3), pat(96, 2), 1)
refusal("line_eval_batch_len_r", "line_eval_batch", pat(192, 1), None, pat(96, 2), 2)
case("final_exp", "final_exp", pat(576, 1))
refusal("final_exp_len", "final_exp", pat(575, 1))
case("final_exp_batch", "final_exp_batch", pat(576 * 2, 1))
refusal("final_exp_batch_len", "final_exp_batch", pat(577, 1))
case("fq12_op_mul", "fq12_op", "mul", pat(576 * 2, 1), pat(576 * 2, 2))
case("fq12_op_inv", "fq12_op", "inv", pat(576, 1))
refusal("fq12_op_len", "fq12_op", "add", pat(576, 1), pat(1152, 2))
refusal("fq12_op_len_a", "fq12_op", "neg", pat(100, 1))
case("fq12_pow", "fq12_pow", pat(576 * 3, 1), 0x1ffff)
case("fq12_pow_zero", "fq12_pow", pat(576, 1), 0)
refusal("fq12_pow_negative", "fq12_pow", pat(576, 1), -1)
refusal("fq12_pow_len", "fq12_pow", pat(100, 1), 5)
case("pairing_multi_batch", "pairing_multi_batch", pat(96 * 6, 1), pat(192 * 6, 2), 2, 3)
case("pairing_multi_batch_inf", "pairing_multi_batch", pat(96 * 2, 1), pat(192 * 2, 2), 1, 2, inf=[0, 0, 0, 1])
refusal("pairing_multi_batch_len", "pairing_multi_batch", pat(96 * 6, 1), pat(192 * 6, 2), 2, 2)

# ---- points in, points out ----
case("g1_decompress", "g1_decompress", pat(48 * 3, 1))
case("g2_decompress", "g2_decompress", pat(96 * 2, 1))
refusal("g1_decompress_len", "g1_decompress", pat(49, 1))
refusal("g2_decompress_len", "g2_decompress", pat(48, 1))
case("hash_to_g2", "hash_to_g2", pat(64, 1))
refusal("hash_to_g2_len", "hash_to_g2", pat(33, 1))
case("map_to_g2", "map_to_g2", pat(192 * 2, 1))
refusal("map_to_g2_len", "map_to_g2", pat(96, 1))
for g, psz in (("g1", 96), ("g2", 192)):
    case(g + "_msm_ints", g + "_msm", pat(psz * 6, 1), ints(6), 3, 2)
    case(g + "_msm_bytes", g + "_msm", pat(psz * 6, 1), be(ints(6)), 3, 2)
    case(g + "_msm_bytearray", g + "_msm", bytearray(pat(psz * 2, 1)), bytearray(be(ints(2))), 2)
    case(g + "_msm_plain", g + "_msm", pat(psz * 2, 1), None, 2)
    refusal(g + "_msm_len", g + "_msm", pat(psz * 2, 1), None, 3)
    refusal(g + "_msm_scalar_len", g + "_msm", pat(psz * 2, 1), ints(3), 2)
    case(g + "_subgroup", g + "_subgroup", pat(psz * 3, 1))
    refusal(g + "_subgroup_len", g + "_subgroup", pat(psz + 1, 1))
    case(g + "_subgroup_dev", g + "_subgroup_dev", 1000, 3, 2000)
    case(g + "_subgroup_dev_stream", g + "_subgroup_dev", 1000, 3, 2000, 77)

# ---- fixed-base multiplication and HD keys ----
for name in ("g1_mul_gen", "g1_mul_gen_secret"):
    case(name + "_ints", name, ints(3))
    case(name + "_bytes", name, be(ints(3)))
    case(name + "_aff", name, ints(2), ser=False)
    case(name + "_ser", name, be(ints(1)), aff=False)
    refusal(name + "_len", name, pat(33, 1))
    refusal(name + "_no_output", name, ints(1), aff=False, ser=False)
case("g1_mul_gen_add_one", "g1_mul_gen", ints(3), pat(96, 4), 1)
case("g1_mul_gen_add_each", "g1_mul_gen", be(ints(2)), bytearray(pat(192, 4)), 2, aff=False)
refusal("g1_mul_gen_add_count", "g1_mul_gen", ints(3), pat(192, 4), 2)
refusal("g1_mul_gen_add_len", "g1_mul_gen", ints(3), pat(95, 4), 1)
refusal("g1_mul_gen_add_missing", "g1_mul_gen", ints(3), None, 1)
case("g1_mul_gen_dev", "g1_mul_gen_dev", 1000, 3, 2000, 3000)
case("g1_mul_gen_dev_add", "g1_mul_gen_dev", 1000, 3, 2000, None, 77, 4000, 1)
case("g1_mul_gen_secret_dev", "g1_mul_gen_secret_dev", 1000, 3, 2000, 3000)
case("g1_mul_gen_secret_dev_stream", "g1_mul_gen_secret_dev", 1000, 3, None, 3000, stream=77)
case("hd_children_private", "hd_children", pat(32, 1), pat(96, 2), pat(32, 3), [0, 1 << 31, (1 << 32) - 1])
case("hd_children_public", "hd_children", pat(32, 1), pat(96, 2), None, [5, 6], ser=False)
case("hd_children_ser", "hd_children", bytearray(pat(32, 1)), bytearray(pat(96, 2)), bytearray(pat(32, 3)), [7], aff=False)
case("hd_children_none", "hd_children", pat(32, 1), pat(96, 2), None, [])
refusal("hd_children_chain_len", "hd_children", pat(31, 1), pat(96, 2), None, [1])
refusal("hd_children_pk_len", "hd_children", pat(32, 1), pat(95, 2), None, [1])
refusal("hd_children_sk_len", "hd_children", pat(32, 1), pat(96, 2), pat(33, 3), [1])
refusal("hd_children_index_high", "hd_children", pat(32, 1), pat(96, 2), None, [1, 1 << 32])
refusal("hd_children_index_negative", "hd_children", pat(32, 1), pat(96, 2), pat(32, 3), [-1])
case("hd_children_dev", "hd_children_dev", pat(32, 1), pat(96, 2), pat(32, 3), 1000, 3, 2000, 3000, 4000, 5000)
case("hd_children_dev_public", "hd_children_dev", bytearray(pat(32, 1)), bytearray(pat(96, 2)), None, 1000, 3, 2000, None, 4000, None, 77)
PARENTS = pat(2 * 160, 9)
case("hd_paths_private", "hd_paths", PARENTS, True, [1, 0, 1], [[1, 1 << 31], [2, 3], [(1 << 32) - 1, 0]])
case("hd_paths_public", "hd_paths", PARENTS, False, None, [[1], [2]], ser=False, fp=False)
case("hd_paths_ser", "hd_paths", bytearray(PARENTS[:160]), True, [0], [[4, 5, 6]], aff=False)
case("hd_paths_none", "hd_paths", PARENTS, True, None, [])
case("hd_paths_none_of", "hd_paths", PARENTS, False, [], [])
case("hd_paths_secret_flag", "hd_paths", PARENTS, True, (1, 1), ((1, 2), (3, 4)), secret=True)
case("hd_paths_secret", "hd_paths_secret", PARENTS, [1, 0, 1], [[1, 1 << 31], [2, 3], [4, 0]])
case("hd_paths_secret_outputs", "hd_paths_secret", PARENTS, None, [[1]], False, True, False)
for name, lead in (("hd_paths", (PARENTS, True)), ("hd_paths_secret", (PARENTS,))):
    refusal(name + "_parent_len", name, PARENTS[:161], *lead[1:], None, [[1]])
    refusal(name + "_depth", name, *lead, None, [[1, 2], [3]])
    refusal(name + "_parent_of_len", name, *lead, [0], [[1], [2]])
    for what, bad in (("high", 1 << 32), ("negative", -1)):
        refusal("%s_index_%s" % (name, what), name, *lead, None, [[1, 2], [3, bad]])
        refusal("%s_parent_of_%s" % (name, what), name, *lead, [0, bad], [[1], [2]])
        NO_MESSAGE.update(("%s_index_%s" % (name, what), "%s_parent_of_%s" % (name, what)))
case("hd_paths_dev", "hd_paths_dev", 1000, 2, True, 1500, 2000, 2, 3, 3000, 4000, 5000, 6000, 7000)
case("hd_paths_dev_public", "hd_paths_dev", 1000, 2, False, None, 2000, 1, 3, 3000, None, 5000, None, None, 77)
case("hd_paths_secret_dev", "hd_paths_secret_dev", 1000, 2, 1500, 2000, 2, 3, 3000, 4000, 5000, 6000, 7000)
case("hd_paths_secret_dev_stream", "hd_paths_secret_dev", 1000, 1, None, 2000, 1, 3, 3000, 4000, None, 6000, None, stream=77)

# ---- Feldman share checks ----
COMMIT = pat(96 * 2 * 3, 1)                  # n_polys = 2, t = 3
for name in ("g1_poly_check", "g1_poly_check_secret"):
    case(name + "_ints", name, COMMIT, 2, 3, [0, 1, 1], ints(3), ints(3, 1))
    case(name + "_bytes", name, bytearray(COMMIT), 2, 3, (1, 0), be(ints(2)), bytearray(be(ints(2, 1))), aff=True)
    refusal(name + "_x_len", name, COMMIT, 2, 3, [0, 1], ints(3), ints(2, 1))
    refusal(name + "_s_len", name, COMMIT, 2, 3, [0, 1], ints(2), ints(1, 1))
    refusal(name + "_commit_len", name, COMMIT, 2, 2, [0], ints(1), ints(1, 1))
    refusal(name + "_index_high", name, COMMIT, 2, 3, [0, 1 << 32], ints(2), ints(2, 1))
    refusal(name + "_index_negative", name, COMMIT, 2, 3, [-1], ints(1), ints(1, 1), True)
    case(name + "_dev", name + "_dev", 1000, 2, 3, 2000, 3000, 4000, 5, 5000, 6000)
    case(name + "_dev_stream", name + "_dev", 1000, 2, 3, 2000, 3000, None, 5, None, 6000, 77)
case("g1_poly_check_evaluate", "g1_poly_check", COMMIT, 2, 3, [1], ints(1), aff=True)
case("g1_poly_check_secret_flag", "g1_poly_check", COMMIT, 2, 3, [1], ints(1), ints(1, 1), secret=True)
refusal("g1_poly_check_no_output", "g1_poly_check", COMMIT, 2, 3, [1], ints(1))
refusal("g1_poly_check_secret_no_s", "g1_poly_check_secret", COMMIT, 2, 3, [1], ints(1), None, True)

# ---- threshold recovery and signature shares ----
for name in ("lagrange_at_zero",):
    case(name + "_ints", name, ints(6), 3, 2)
    case(name + "_bytes", name, be(ints(2)), 2)
    refusal(name + "_len", name, ints(5), 3, 2)
    case(name + "_dev", name + "_dev", 1000, 3, 2, 2000, 3000)
    case(name + "_dev_stream", name + "_dev", 1000, 3, 2, 2000, 3000, 77)
for name in ("fr_interpolate_at_zero", "fr_interpolate_at_zero_secret"):
    case(name + "_ints", name, ints(6), ints(6, 1), 3, 2)
    case(name + "_bytes", name, be(ints(2)), bytearray(be(ints(2, 1))), 2)
    refusal(name + "_x_len", name, ints(5), ints(6, 1), 3, 2)
    refusal(name + "_y_len", name, ints(6), be(ints(5, 1)), 3, 2)
    case(name + "_dev", name + "_dev", 1000, 1500, 3, 2, 2000, 3000)
    case(name + "_dev_stream", name + "_dev", 1000, 1500, 3, 2, 2000, 3000, 77)
case("threshold_combine_ints", "threshold_combine", pat(192 * 6, 1), ints(6), 3, 2)
case("threshold_combine_bytes", "threshold_combine", bytearray(pat(192 * 2, 1)), be(ints(2)), 2)
refusal("threshold_combine_len", "threshold_combine", pat(192 * 5, 1), ints(6), 3, 2)
refusal("threshold_combine_x_len", "threshold_combine", pat(192 * 6, 1), ints(5), 3, 2)
case("threshold_combine_dev", "threshold_combine_dev", 1000, 1500, 3, 2, 2000, 2500, 3000)
case("threshold_combine_dev_stream", "threshold_combine_dev", 1000, 1500, 3, 2, 2000, None, 3000, 77)
SHARES = (pat(192 * 6, 1), pat(96 * 4, 2), [0, 3, 1, 2, 2, 0], ints(6), pat(64, 3))
WEIGHTS = [1, 0, (1 << 64) - 1, 5, 6, 7]
case("sig_shares_check_ints", "sig_shares_check", *SHARES, WEIGHTS, 3, 2)
case("sig_shares_check_bytes", "sig_shares_check", bytearray(SHARES[0]), bytearray(SHARES[1]), tuple(SHARES[2]), be(SHARES[3]),
     bytearray(SHARES[4]), bytearray(be(WEIGHTS, 8)), 3, 2)
case("sig_shares_check_plain", "sig_shares_check", pat(192 * 2, 1), pat(96, 2), [0, 0], None, pat(32, 3), [1, 2], 2, scaled=False)
case("sig_shares_check_plain_x", "sig_shares_check", pat(192, 1), pat(96, 2), [0], "ignored", pat(32, 3), [1], 1, 1, False)
refusal("sig_shares_check_sigs_len", "sig_shares_check", SHARES[0][:-1], *SHARES[1:], WEIGHTS, 3, 2)
refusal("sig_shares_check_keys_len", "sig_shares_check", SHARES[0], pat(95, 2), *SHARES[2:], WEIGHTS, 3, 2)
refusal("sig_shares_check_idx_len", "sig_shares_check", *SHARES[:2], [0, 1], *SHARES[3:], WEIGHTS, 3, 2)
refusal("sig_shares_check_hash_len", "sig_shares_check", *SHARES[:4], pat(32, 3), WEIGHTS, 3, 2)
refusal("sig_shares_check_weights_len", "sig_shares_check", *SHARES, WEIGHTS[:5], 3, 2)
refusal("sig_shares_check_x_len", "sig_shares_check", *SHARES[:3], ints(5), SHARES[4], WEIGHTS, 3, 2)
refusal("sig_shares_check_no_x", "sig_shares_check", *SHARES[:3], None, SHARES[4], WEIGHTS, 3, 2)
refusal("sig_shares_check_index_high", "sig_shares_check", *SHARES[:2], [0, 1, 2, 3, 1 << 32, 0], *SHARES[3:], WEIGHTS, 3, 2)
refusal("sig_shares_check_index_negative", "sig_shares_check", *SHARES[:2], [0, 1, 2, 3, -1, 0], *SHARES[3:], WEIGHTS, 3, 2)
case("sig_shares_check_dev", "sig_shares_check_dev", 1000, 1500, 4, 2000, 2500, 3000, 3500, True, 3, 2, 4000, 4500)
case("sig_shares_check_dev_plain", "sig_shares_check_dev", 1000, 1500, 4, 2000, None, 3000, 3500, False, 3, 2, 4000, 4500, 77)

# ---- secret scalars: G2 multiplication, signing, dealing, sums ----
case("g2_mul_secret_ints", "g2_mul_secret", pat(192 * 3, 1), ints(3))
case("g2_mul_secret_one_point", "g2_mul_secret", bytearray(pat(192, 1)), be(ints(2)), ser=False)
case("g2_mul_secret_ser", "g2_mul_secret", pat(192, 1), bytearray(be(ints(1))), aff=False)
refusal("g2_mul_secret_len", "g2_mul_secret", pat(191, 1), ints(1))
refusal("g2_mul_secret_scalar_len", "g2_mul_secret", pat(192, 1), pat(31, 1))
refusal("g2_mul_secret_no_output", "g2_mul_secret", pat(192, 1), ints(1), False, False)
case("g2_mul_secret_dev", "g2_mul_secret_dev", 1000, 1, 2000, 3, 3000, 4000)
case("g2_mul_secret_dev_inf", "g2_mul_secret_dev", 1000, 3, 2000, 3, None, 4000, 5000, 77)
case("sign_ints", "sign", ints(3), pat(96, 1))
case("sign_one_hash", "sign", be(ints(2)), bytearray(pat(32, 1)), ser=False)
case("sign_ser", "sign", bytearray(be(ints(1))), pat(32, 1), aff=False)
refusal("sign_len", "sign", pat(33, 1), pat(32, 1))
refusal("sign_hash_len", "sign", ints(1), pat(31, 1))
refusal("sign_no_output", "sign", ints(1), pat(32, 1), False, False)
case("sign_dev", "sign_dev", 1000, 2000, 1, 3, 3000, 4000)
case("sign_dev_stream", "sign_dev", 1000, 2000, 3, 3, None, 4000, 77)
case("threshold_deal_secret_ints", "threshold_deal_secret", ints(6), 3, ints(2, 1))
case("threshold_deal_secret_bytes", "threshold_deal_secret", be(ints(2)), 2, bytearray(be(ints(3, 1))), commit=False)
case("threshold_deal_secret_commit", "threshold_deal_secret", bytearray(be(ints(3))), 1, "ignored", frag=False)
refusal("threshold_deal_secret_t", "threshold_deal_secret", ints(2), 0, ints(1))
refusal("threshold_deal_secret_len", "threshold_deal_secret", ints(5), 3, ints(1))
refusal("threshold_deal_secret_x_len", "threshold_deal_secret", ints(3), 3, pat(33))
refusal("threshold_deal_secret_no_output", "threshold_deal_secret", ints(3), 3, ints(1), False, False)
case("threshold_deal_secret_dev", "threshold_deal_secret_dev", 1000, 2, 3, 2000, 4, 3000, 4000)
case("threshold_deal_secret_dev_stream", "threshold_deal_secret_dev", 1000, 2, 3, None, 0, 3000, None, 77)
case("fr_sum_secret_ints", "fr_sum_secret", ints(6), 3, 2)
case("fr_sum_secret_pk", "fr_sum_secret", be(ints(2)), 2, pk=True)
case("fr_sum_secret_aff", "fr_sum_secret", bytearray(be(ints(3))), 1, 3, aff=True)
case("fr_sum_secret_ser", "fr_sum_secret", ints(1), 1, 1, False, False, True)
refusal("fr_sum_secret_k", "fr_sum_secret", [], 0)
refusal("fr_sum_secret_len", "fr_sum_secret", ints(5), 3, 2)
case("fr_sum_secret_dev", "fr_sum_secret_dev", 1000, 3, 2, 2000, 3000, 4000)
case("fr_sum_secret_dev_stream", "fr_sum_secret_dev", 1000, 3, 2, 2000, None, None, 77)
case("sign_threshold_ints", "sign_threshold", ints(6), ints(6, 1), 3, pat(64, 1), 2)
case("sign_threshold_one_hash", "sign_threshold", be(ints(2)), bytearray(be(ints(2, 1))), 2, bytearray(pat(32, 1)), ser=False)
case("sign_threshold_ser", "sign_threshold", ints(1), ints(1, 1), 1, pat(32, 1), 1, False)
refusal("sign_threshold_hash_len", "sign_threshold", ints(1), ints(1, 1), 1, pat(33, 1))
refusal("sign_threshold_no_output", "sign_threshold", ints(1), ints(1, 1), 1, pat(32, 1), 1, False, False)
refusal("sign_threshold_sks_len", "sign_threshold", ints(2), ints(1, 1), 1, pat(32, 1))
refusal("sign_threshold_x_len", "sign_threshold", ints(1), ints(2, 1), 1, pat(32, 1))
case("sign_threshold_dev", "sign_threshold_dev", 1000, 1500, 3, 2, 2000, 1, 3000, 4000, 5000, 6000)
case("sign_threshold_dev_stream", "sign_threshold_dev", 1000, 1500, 3, 2, 2000, 2, None, 4000, None, 6000, 77)

# ---- secure aggregation: the digests come from the caller, from the host (few groups) or from the device ----
PKS = pat(48 * 6, 1)                         # groups = 2, k = 3
DIGESTS = pat(64, 5)
case("hash_pks_host_digest", "hash_pks", PKS, 3, 2, 2)
case("hash_pks_device_digest", "hash_pks", bytearray(PKS), 3, 1, 2, pk_hash=False)
case("hash_pks_given_digest", "hash_pks", PKS, 3, 3, 2, bytearray(DIGESTS), True)
case("hash_pks_want_digest", "hash_pks", PKS[:48], 1, 1, want_pk_hash=True)
case("hash_pks_many_groups", "hash_pks", pat(48 * _native.HASH_PKS_DEVICE_GROUPS, 1), 1, 1, _native.HASH_PKS_DEVICE_GROUPS)
refusal("hash_pks_len", "hash_pks", PKS, 2, 1, 2)
refusal("hash_pks_digest_len", "hash_pks", PKS, 3, 1, 2, pat(32, 5))
case("aggregate_pub_keys_secure", "aggregate_pub_keys_secure", pat(96 * 6, 2), PKS, 3, 2)
case("aggregate_pub_keys_secure_device", "aggregate_pub_keys_secure", bytearray(pat(96 * 6, 2)), bytearray(PKS), 3, 2, False)
case("aggregate_pub_keys_secure_given", "aggregate_pub_keys_secure", pat(96 * 6, 2), PKS, 3, 2, pk_hash=DIGESTS)
refusal("aggregate_pub_keys_secure_len", "aggregate_pub_keys_secure", pat(96 * 5, 2), PKS, 3, 2)
refusal("aggregate_pub_keys_secure_pks_len", "aggregate_pub_keys_secure", pat(96 * 6, 2), PKS[:-1], 3, 2)
refusal("aggregate_pub_keys_secure_digest_len", "aggregate_pub_keys_secure", pat(96 * 6, 2), PKS, 3, 2, pat(63))
case("aggregate_sigs_secure", "aggregate_sigs_secure", pat(192 * 4, 2), 2, PKS, 3, 2)
case("aggregate_sigs_secure_device", "aggregate_sigs_secure", bytearray(pat(192 * 2, 2)), 1, bytearray(PKS), 3, 2, False)
case("aggregate_sigs_secure_given", "aggregate_sigs_secure", pat(192 * 3, 2), 3, PKS[:144], 3, pk_hash=DIGESTS[:32])
refusal("aggregate_sigs_secure_len", "aggregate_sigs_secure", pat(192 * 3, 2), 2, PKS, 3, 2)
refusal("aggregate_sigs_secure_pks_len", "aggregate_sigs_secure", pat(192 * 4, 2), 2, PKS, 2, 2)
refusal("aggregate_sigs_secure_digest_len", "aggregate_sigs_secure", pat(192 * 4, 2), 2, PKS, 3, 2, pat(65))
case("aggregate_priv_keys_secure_ints", "aggregate_priv_keys_secure", ints(6), PKS, 3, 2)
case("aggregate_priv_keys_secure_pk", "aggregate_priv_keys_secure", be(ints(6)), bytearray(PKS), 3, 2, True, pk_hash=False)
case("aggregate_priv_keys_secure_aff", "aggregate_priv_keys_secure", bytearray(be(ints(3))), PKS[:144], 3, aff=True, pk_hash=DIGESTS[:32])
case("aggregate_priv_keys_secure_ser", "aggregate_priv_keys_secure", ints(1), PKS[:48], 1, 1, False, False, True)
refusal("aggregate_priv_keys_secure_len", "aggregate_priv_keys_secure", ints(5), PKS, 3, 2)
refusal("aggregate_priv_keys_secure_pks_len", "aggregate_priv_keys_secure", ints(6), PKS, 2, 2)
refusal("aggregate_priv_keys_secure_digest_len", "aggregate_priv_keys_secure", ints(6), PKS, 3, 2, pk_hash=pat(1))
case("hash_pks_dev", "hash_pks_dev", 1000, 3, 2, 1500, 2, 2000)
case("hash_pks_dev_digest", "hash_pks_dev", None, 3, 2, 1500, 2, 2000, 2500, 77)
case("aggregate_pub_keys_secure_dev", "aggregate_pub_keys_secure_dev", 1000, 1500, None, 3, 2, 2000)
case("aggregate_pub_keys_secure_dev_inf", "aggregate_pub_keys_secure_dev", 1000, None, 1700, 3, 2, 2000, 2500, 77)
case("aggregate_sigs_secure_dev", "aggregate_sigs_secure_dev", 1000, 2, 1500, 3, None, 2, 2000)
case("aggregate_sigs_secure_dev_inf", "aggregate_sigs_secure_dev", 1000, 2, None, 3, 1700, 2, 2000, 2500, 77)
case("aggregate_priv_keys_secure_dev", "aggregate_priv_keys_secure_dev", 1000, 1500, None, 3, 2, 2000)
case("aggregate_priv_keys_secure_dev_pk", "aggregate_priv_keys_secure_dev", 1000, None, 1700, 3, 2, 2000, 2500, 3000, 77)

# ---- device-pointer forms of the pairing path: stream comes before d_inf in Python, after it in C ----
for name in ("pairing_multi_dev", "miller_loop_batch_dev", "miller_product_dev"):
    case(name, name, 1000, 2000, 3, 3000)
    case(name + "_inf", name, 1000, 2000, 3, 3000, 77, 4000)
for name in ("pairing_multi_batch_dev", "miller_product_batch_dev"):
    case(name, name, 1000, 2000, 2, 3, 3000)
    case(name + "_inf", name, 1000, 2000, 2, 3, 3000, 77, 4000)
case("final_exp_product_dev", "final_exp_product_dev", 1000, 3, 2000)
case("final_exp_product_dev_stream", "final_exp_product_dev", 1000, 3, 2000, 77)
case("final_exp_product_batch_dev", "final_exp_product_batch_dev", 1000, 3, 2, 2000)
case("final_exp_product_batch_dev_stream", "final_exp_product_batch_dev", 1000, 3, 2, 2000, 77)


def run_case(method, args, kwargs):
    """-> {"calls": what the library saw, "returns": the shape of the result} or {"raises": type, "message": text}"""
    e = stub_engine()
    try:
        r = getattr(e, method)(*args, **kwargs)
    except Exception as x:
        assert not e.lib.calls, "a refused call must not reach the library"
        return {"raises": type(x).__name__, "message": str(x)}
    finally:
        calls, e.lib.calls, e.h = list(e.lib.calls), [], None          # (h = None: the stub engine's __del__ has nothing to close)
    return {"calls": calls, "returns": _shape(r)}


def public_methods(cls):
    return sorted(n for n, v in vars(cls).items() if not n.startswith("_") and callable(v))


def test_every_public_engine_method_has_a_case():
    assert sorted({c[1] for c in CASES}) == public_methods(_native.Engine)


@pytest.mark.parametrize("cid,method,args,kwargs", CASES, ids=[c[0] for c in CASES])
def test_engine_call(cid, method, args, kwargs):
    want = load_golden(RECORDS)["engine"][cid]
    got = run_case(method, args, kwargs)
    assert ("raises" in got) == (cid in REFUSALS)
    if cid in NO_MESSAGE:
        got["message"] = None
    assert json.loads(json.dumps(got)) == want


def test_refusals_the_issue_names_are_pinned():
    """the index refusals are OverflowError for 1 << 32 and for -1, everywhere an index array is built"""
    rec = load_golden(RECORDS)["engine"]
    names = [n + s for n in ("hd_children", "g1_poly_check", "g1_poly_check_secret", "sig_shares_check") for s in ("_index_high", "_index_negative")]
    names += [n + m + s for n in ("hd_paths", "hd_paths_secret") for m in ("_index", "_parent_of") for s in ("_high", "_negative")]
    assert all(rec[n]["raises"] == "OverflowError" for n in names)
    assert rec["g1_poly_check_secret_no_s"]["raises"] == rec["fr_sum_secret_k"]["raises"] == "ValueError"


# ---- HipProvider over a stub engine: every method hands on the arguments it is given and returns the engine's result ----
PROVIDER_ARGS = {                            # method: the number of arguments the scheme code may pass (all of them are passed here)
    "pairing_multi": 4, "miller_loop_batch": 4, "line_eval_batch": 4, "final_exp": 1, "pairing_multi_batch": 5, "g1_msm": 4, "g2_msm": 4,
    "map_to_g2": 1, "hash_to_g2": 1, "g1_decompress": 1, "g2_decompress": 1, "g1_mul_gen": 3, "hd_children": 4, "hd_paths": 4,
    "g1_mul_gen_secret": 1, "hd_paths_secret": 3, "g1_poly_check": 7, "g1_subgroup": 1, "g2_subgroup": 1, "lagrange_at_zero": 3,
    "fr_interpolate_at_zero": 4, "threshold_combine": 4, "sig_shares_check": 9, "g2_mul_secret": 4, "sign": 4, "threshold_deal_secret": 5,
    "fr_interpolate_at_zero_secret": 4, "g1_poly_check_secret": 7, "fr_sum_secret": 4, "sign_threshold": 7, "hash_pks": 4,
    "aggregate_pub_keys_secure": 4, "aggregate_sigs_secure": 5, "aggregate_priv_keys_secure": 5, "verify_pipeline": 8,
}


class StubEngine:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args, **kwargs):
            self.calls.append((name, args, kwargs))
            return ("result of", name)
        return fn


def stub_provider():
    p = backend.HipProvider.__new__(backend.HipProvider)
    p._eng = StubEngine()
    return p


def test_provider_names():
    """the scheme code chooses its path by hasattr(provider, name): the names present are exactly these"""
    p = stub_provider()
    assert sorted(n for n in dir(p) if not n.startswith("_")) == sorted(list(PROVIDER_ARGS) + ["LAGRANGE_MAX_K"])
    assert p.LAGRANGE_MAX_K == _native.LAGRANGE_MAX_K == 1024
    assert not hasattr(p, "hd_paths_dev") and getattr(p, "close", None) is None


@pytest.mark.parametrize("name", sorted(PROVIDER_ARGS))
def test_provider_forwards(name):
    p = stub_provider()
    args = tuple(object() for _ in range(PROVIDER_ARGS[name]))
    assert getattr(p, name)(*args) == ("result of", name)
    (called, got, kwargs), = p._eng.calls
    assert called == name and not kwargs and len(got) == len(args) and all(a is b for a, b in zip(got, args))


def test_provider_arguments_are_the_engines():
    """every argument the provider takes is one the engine method of that name takes, in that order"""
    import inspect
    for name, count in PROVIDER_ARGS.items():
        assert len(inspect.signature(getattr(_native.Engine, name)).parameters) - 1 >= count, name


if __name__ == "__main__":
    records = {}
    for cid, method, args, kwargs in CASES:
        records[cid] = json.loads(json.dumps(run_case(method, args, kwargs)))
        if cid in NO_MESSAGE:
            records[cid]["message"] = None
    with open(os.path.join(GOLDEN, RECORDS), "w") as f:
        json.dump({"engine": records}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d records -> %s" % (len(records), os.path.join(GOLDEN, RECORDS)), file=sys.stderr)
