"""Integer model of the scalar-independent fixed-base G1 multiplication (csrc/blsgpu_g1fix.hip k_fix_table_t<4> /
k_fix_mul_secret): the SPECIFICATION of its table and of its schedule.  out = s G1 for the literal integer s < 2^256 (G1 has
order n, so this is (s mod n) G1, the value of k_fix_mul), computed so that WHAT is done and WHICH table entries are touched
is the same for every s -- what that claims and what it does not is stated once, in csrc/secret_window.h.

  recode(s)      g2smul_model's, as are WINDOWS and TABLE: signed 4-bit digits d_w in [-8, 8), 65 windows.
  build_table()  T[w][e] = (e + 1) 16^w G1 for w < 65, e < 8 -- 520 affine points, built once per context.  The base point
                 is fixed and public, so the powers of 16 are in the table and the schedule has NO doubling.
  mul_gen(s)     for every window, least significant first: READ ALL EIGHT entries of the window and keep T[w][|d| - 1]
                 (d = 0: entry 0), negated for d < 0; ONE mixed addition of it; for d = 0 the sum is dropped and the old
                 accumulator kept (an affine addend cannot be infinity, so a zero digit adds entry 0 all the same).
                 65 additions whatever the scalar.

Every step appends (operation, entries read) to a trace; the trace is what must not depend on the scalar
(tests/test_g1fixs_model.py compares it with == across scalars).  The VALUE kept by a select is data, not schedule: it does
not appear in the trace, as it does not appear in the device's instruction stream or addresses.
"""
from bls_py import hostmath as H
from .g2smul_model import TABLE, WINDOWS, recode

ENTRY_BYTES = 112                                         # affine (x, y) in L28 form: 2 x 14 limbs of 4 bytes
TABLE_BYTES = WINDOWS * TABLE * ENTRY_BYTES


def build_table():
    """T[w][e] = (e + 1) 16^w G1 as Jacobian points; k_fix_table_t<4>"""
    T = []
    base = H.aff_to_jac(H.F1, H.G1_GEN)
    for _ in range(WINDOWS):
        row = [base]
        for _e in range(1, TABLE):
            row.append(H.jac_add(H.F1, row[-1], base))
        T.append(row)
        base = H.jac_double(H.F1, row[TABLE - 1])         # 16 * base
    return T


def mul_gen(s, table):
    """(s G1 as an affine point or None, trace) on build_table()'s table"""
    trace = []
    acc = None
    for w, d in enumerate(recode(s)):
        trace.append(("select", tuple((w, e) for e in range(TABLE))))      # all eight are read; one is kept by value
        E = table[w][abs(d) - 1 if d else 0]
        added = H.jac_add(H.F1, acc, E if d >= 0 else H.jac_neg(H.F1, E))
        trace.append(("madd", ()))
        acc = added if d else acc                          # a select per limb, not a branch
        trace.append(("keep", ()))
    return H.jac_to_affine(H.F1, acc), trace
