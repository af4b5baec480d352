"""Integer model of the scalar-independent G2 multiplication (csrc/blsgpu_g2smul.hip k_g2_smul_table / k_g2_smul): the
SPECIFICATION of its schedule.  out = s P for the literal integer s < 2^256 (no reduction mod the group order, as the
`scalars` of blsgpu_g2_msm), computed so that WHAT is done and WHICH table entries are touched is the same for every s.
What that claims and what it does not is stated once, in csrc/secret_window.h.

Two parts:

  recode(s)      signed 4-bit digits by the sorted sums' trick (blsgpu_msm.hip): the nibbles of s + C, C = sum_w 8 16^w over
                 WINDOWS = 65 windows, minus 8 -- d_w in [-8, 8) with sum_w d_w 16^w = s.  s + C < 16^65 for every s < 2^256,
                 so there is no carry out and no case split; the device does it with nine additions with carry.
  smul(P, s)     the window schedule on exact point arithmetic (bls_py.hostmath, Jacobian; None = infinity): a table
                 T[e] = (e + 1) P, e < 8, built by seven additions of P; then from the top window down four doublings and ONE
                 addition of the selected entry -- every window READS ALL EIGHT entries and keeps T[|d| - 1], negated for
                 d < 0, or infinity for d = 0 (the device: the constant (0 : 1 : 0), a no-op of the complete addition).
                 260 doublings and 65 additions whatever the scalar.

Every step appends (operation, table indices read, table index written) to a trace; the trace is what must not depend on
the scalar (tests/test_g2smul_model.py compares it with == across scalars, with a table per scalar and with a shared one).
The VALUE kept by a select is data, not schedule: it does not appear in the trace, as it does not appear in the device's
instruction stream or addresses.
"""
from bls_py import hostmath as H

WINDOWS = 65
TABLE = 8
BIAS = sum(8 << (4 * w) for w in range(WINDOWS))         # C
ALL = tuple(range(TABLE))


def recode(s):
    """digits d_w in [-8, 8), least significant first"""
    if not 0 <= s < 1 << 256:
        raise ValueError("scalars are 256-bit")
    t = s + BIAS
    assert t < 1 << (4 * WINDOWS)
    return [((t >> (4 * w)) & 15) - 8 for w in range(WINDOWS)]


def build_table(P, trace=None):
    """T[e] = (e + 1) P for the affine point P (None = infinity) as Jacobian points; k_g2_smul_table"""
    trace = [] if trace is None else trace
    J = H.aff_to_jac(H.F2, P)
    T = [J]
    trace.append(("load", (), 0))
    for e in range(1, TABLE):
        T.append(H.jac_add(H.F2, T[e - 1], J))
        trace.append(("table_add", (e - 1, 0), e))
    return T, trace


def smul(P, s, table=None):
    """(s P as an affine point or None, trace).  table: a shared table of P (build_table), else one is built here and its
    steps head the trace."""
    trace = []
    T = table if table is not None else build_table(P, trace)[0]
    digits = recode(s)
    acc = None
    for w in range(WINDOWS - 1, -1, -1):
        for _ in range(4):
            acc = H.jac_double(H.F2, acc)
            trace.append(("dbl", (), None))
        d = digits[w]
        trace.append(("select", ALL, None))               # all eight are read; one is kept by value
        Q = None if d == 0 else (T[abs(d) - 1] if d > 0 else H.jac_neg(H.F2, T[abs(d) - 1]))
        acc = H.jac_add(H.F2, acc, Q)
        trace.append(("add", (), None))
    return H.jac_to_affine(H.F2, acc), trace
