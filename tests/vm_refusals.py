"""Calls of the VM check library that its host side must refuse before anything is launched (csrc/vm_check_plan.h verify()), and a
few it must accept, shared by tests/test_vm_check_host.py (the decision, compiled for the CPU) and tests/test_gpu_vm.py (the library).
Each case: (name, op code, input words, teams, output words, expected return code)."""
import vm_vectors as V

INACTIVE = V.INACTIVE


def _base(nslots=40):
    p = V.Program("base", "refusal", nslots)
    p.mul({0: (1, 2, 3), 5: (4, 4, 6)})
    p.lin({0: (7, 1 << 14, [(3, 1)], [(2, 2), (1, 3)]), 1: (None, 0, [], [(5, 4)]), 9: (8, 0, [(1, 5)], [])})
    p.unary("inv", {2: (3, 9)})
    return p


def _words(p, n=1, tpw=1, rounds=None, table=None, nslots=None, check_at=0, chk_slot=0):
    nslots = nslots or p.nslots
    imgs = [[(s + 1) % V.Q for s in range(nslots)]] * n
    return V.call_words(rounds if rounds is not None else p.rounds, table if table is not None else p.table(), nslots, imgs, tpw, check_at, chk_slot)


def cases():
    p = _base()
    out = []

    def add(name, want, op="RUN_FULL", n=1, nout=None, **kw):
        nslots = kw.get("nslots") or p.nslots
        w = kw.pop("words", None) or _words(p, n=n, **kw)
        out.append((name, V.OPS[op] if isinstance(op, str) else op, w, n, nout if nout is not None else n * (nslots * 12 + V.TRAILER), want))

    def table_with(at, value):
        t = list(p.table())
        t[at] = value
        return t

    def rounds_with(i, off=None, meta=None):
        r = list(p.rounds)
        r[i] = (off if off is not None else r[i][0], meta if meta is not None else r[i][1])
        return r
    mul_off, lin_off, inv_off = (r[0] for r in p.rounds)
    lin_meta = p.rounds[1][1]
    K = (lin_meta >> 8) & 255
    rl = V.kpad(K)
    add("accepted", 0)
    add("accepted, four teams", 0, n=4, tpw=4)
    add("unknown op", -1, op=9)
    add("one output word short", -2, nout=p.nslots * 12 + V.TRAILER - 1)
    add("teams not a multiple of the workgroup's", -2, n=2, tpw=4)
    add("teams per workgroup 3", -2, n=3, tpw=3)
    add("no rounds", -2, rounds=[])
    add("data_off not a multiple of 4", -4, rounds=rounds_with(0, off=2))
    add("records pass the table", -4, rounds=rounds_with(0, off=len(p.table()) - 252))
    add("records end with the table", 0, rounds=rounds_with(0, off=len(p.table()) - 256))
    add("a LIN round's records pass the table", -4, rounds=rounds_with(1, off=len(p.table()) - 64 * rl + 4))
    add("K = 0", -4, rounds=rounds_with(1, meta=lin_meta & ~(255 << 8)))
    add("K = 30, every lane inactive", 0, rounds=[(0, 1 | (30 << 8))], table=([INACTIVE] + [0] * 31) * 64)
    add("K = 31", -4, rounds=[(0, 1 | (31 << 8))], table=([INACTIVE] + [0] * 35) * 64)
    add("MN > K", -4, rounds=rounds_with(1, meta=(lin_meta & ~(255 << 18)) | ((K + 1) << 18)))
    add("levels 3", -4, rounds=rounds_with(1, meta=lin_meta | (3 << 16)))
    add("a micro-op's slot is nslots", -4, table=table_with(lin_off + 2, (3 << 10) | p.nslots))
    add("a micro-op of an inactive lane names slot nslots", -4, table=table_with(lin_off + 5 * rl + 2, (1 << 10) | p.nslots))
    add("a micro-op with bit 15", -4, table=table_with(lin_off + 2, (1 << 15) | (3 << 10) | 1))
    add("a padding micro-op past K is not looked at", 0, table=table_with(lin_off + 2 + K, 1023))
    add("merge flags with a low bit", -4, table=table_with(lin_off + 1, (1 << 14) | 1))
    add("a MUL operand at 3 nslots", -4, table=table_with(mul_off, 3 * p.nslots))
    add("the operand of an inactive MUL lane at 3 nslots", -4, table=table_with(mul_off + 4 * 7 + 1, 3 * p.nslots))
    add("a MUL operand that is no multiple of 3", -4, table=table_with(mul_off + 1, 4))
    add("a destination that is no multiple of 3", -4, table=table_with(mul_off + 2, 10))
    add("a destination at 3 nslots", -4, table=table_with(mul_off + 2, 3 * p.nslots))
    add("a LIN destination at 3 nslots", -4, table=table_with(lin_off, 3 * p.nslots))
    add("two live MUL lanes with one destination", -4, table=table_with(mul_off + 4 * 5 + 2, 9))
    add("two live LIN lanes with one destination", -4, table=table_with(lin_off + 9 * rl, 21))
    add("an INV operand at 3 nslots", -4, table=table_with(inv_off + 4 * 2, 3 * p.nslots))
    add("a MUL header with K bits", -4, rounds=rounds_with(0, meta=1 << 8))
    add("a window with K + 12 > nslots", -4, op="RUN_LIGHT_STASH", rounds=rounds_with(2, off=0, meta=2 | ((p.nslots - 11) << 8)))
    add("the last window that fits", 0, op="RUN_LIGHT_STASH", rounds=rounds_with(2, off=0, meta=3 | ((p.nslots - 12) << 8)))
    add("a window header whose look-ahead fetch passes the table", -4, op="RUN_LIGHT", rounds=rounds_with(2, off=len(p.table()) - 252, meta=2))
    add("check_at above the limit", -4, op="RUN_FULL_CHK", check_at=V.MAX_ROUNDS + 1)
    add("check_at at the limit", 0, op="RUN_FULL_CHK", check_at=V.MAX_ROUNDS)
    add("the functor's slot is nslots", -4, op="RUN_LIGHT_CHK", rounds=p.rounds[:2], chk_slot=p.nslots)
    # sizes that follow from the header: nr above the limit and nslots above 1023 are refused whatever the buffer holds
    w = _words(p)
    out.append(("nr above the limit", 0, [V.MAX_ROUNDS + 1] + w[1:], 1, p.nslots * 12 + V.TRAILER, -4))
    out.append(("nslots 1024", 0, [w[0], 1024] + w[2:], 1, p.nslots * 12 + V.TRAILER, -4))
    # the LDS a geometry may ask for: 65536 bytes
    big = V.Program("big", "refusal", 342)
    big.mul({0: (1, 2, 3)})
    out.append(("four teams of 342 slots", 0, _words(big, n=4, tpw=4), 4, 4 * (342 * 12 + V.TRAILER), -4))
    ok = V.Program("fits", "refusal", 341)
    ok.mul({0: (1, 2, 3)})
    out.append(("four teams of 341 slots", 0, _words(ok, n=4, tpw=4), 4, 4 * (341 * 12 + V.TRAILER), 0))
    out.append(("eight teams of 171 slots", 0, _words(V.Program("b8", "refusal", 171).mul({0: (1, 2, 3)}), n=8, tpw=8), 8, 8 * (171 * 12 + V.TRAILER), -4))
    return out
