"""CPU: the programs and the word machine of tests/vm_vectors.py (what tests/test_gpu_vm.py holds run_rounds against) checked
against vmgen/tablesim.py, the contract of every synthetic LIN round, and the mutants of the word machine.  Needs no GPU."""
import pytest

import fp28_vectors as F28
import vm_vectors as V
from vmgen import emit

Q = V.Q


def _run(p, op, imgs, **kw):
    m = V.WordMachine(p.table(), imgs, **kw)
    rounds = p.rounds
    check_at, slot = p.check if p.check else (0, 0)
    res = m.run(rounds, op, check_at, slot)
    return m.teams, res


def _agrees(p, op, mutant=None, exact=False):
    """does the word machine (with a mutant) give tablesim's residues, return values, call counts and stash on every image"""
    nteams = 8 if mutant == "base_ignored" else p.nimg
    imgs = [p.images[t % p.nimg] for t in range(nteams)]
    teams, res = _run(p, op, imgs, mutant=mutant, exact=exact)
    for t in range(nteams):
        want, stash, ret, calls = V.reference(p, op, imgs[t])
        if [v % Q for v in teams[t]] != want or (res[t][0], res[t][1]) != (ret, calls):
            return False
        if any(v >= 2 * Q for v in teams[t]):
            return False
        if stash is not None:
            got = [V.F32.from_words(res[t][2][12 * k:12 * k + 12]) % Q for k in range(12)]
            if got != stash or any(res[t][2][144:]):
                return False
    return True


@pytest.fixture(scope="module")
def programs():
    return V.programs()


def test_closed_form_of_the_vm_product_is_the_column_model():
    for cls, w in F28.OPS["b_vm_mul28"].sets:
        A, B = F28.from_words(w[:12]), F28.from_words(w[12:])
        assert F28.vm_mul28_closed(A, B) == F28.vm_mul28(A, B), cls
    for v in V.CLASS_VALUES:
        for u in V.CLASS_VALUES:
            assert F28.vm_mul28_closed(u, v) == F28.vm_mul28(u, v)


def test_word_machine_is_tablesim_on_every_synthetic_program(programs):
    """with the limb models themselves (exact) on the first image and on packed integers on all: the same words, tablesim's residues"""
    for p in programs:
        for op in p.ops:
            assert _agrees(p, op), (p.name, op)
        op = p.ops[0]
        exact, _ = _run(p, op, p.images[:1], exact=True)
        fast, _ = _run(p, op, p.images[:1])
        assert exact == fast, p.name


def test_every_synthetic_round_is_inside_the_lin_contract(programs):
    nlin = 0
    for p in programs:
        for plan, mn in p.plans:
            emit.check_lin_bounds(plan, mn)
            nlin += 1
        assert len(p.plans) == sum(1 for o, m in p.rounds if m & 3 == 1)
    assert nlin > 200


def test_the_classes_hold_what_they_claim(programs):
    by = {c: [p for p in programs if p.cls == c] for c in V.CLASSES}
    metas = lambda ps: [m for p in ps for o, m in p.rounds]
    # lengths: 1 .. 5, one odd and one even above 8, every kind first and last
    assert sorted(set(len(p.rounds) for p in by["lengths"])) == [1, 2, 3, 4, 5, 9, 12]
    for nr in (2, 9, 12):
        ps = [p for p in by["lengths"] if len(p.rounds) == nr]
        assert set(p.rounds[0][1] & 3 for p in ps) == {0, 1, 2, 3} and set(p.rounds[-1][1] & 3 for p in ps) == {0, 1, 2, 3}
    # LIN shape: every K with MN in {0, 1, K - 1, K}
    shapes = set(((m >> 8) & 255, (m >> 18) & 255) for m in metas(by["lin_shape"]) if m & 3 == 1)
    for K in range(1, 31):
        assert {(K, 0), (K, min(1, K)), (K, K - 1), (K, K)} <= shapes, K
    assert any(sum(cf for n, cf, s in negs) == emit.NEG_CF_MAX for p in by["lin_shape"] for plan, mn in p.plans for d, f, negs, poss in plan)
    assert any(p.nslots == 1023 and 1022 in V.referenced_slots(p.rounds, p.table(), False) for p in by["lin_shape"])
    # groups: levels 0, 1, 2; an all-inactive round of either kind
    assert set((m >> 16) & 3 for m in metas(by["groups"]) if m & 3 == 1) == {0, 1, 2}
    # stash: the windows
    wins = set((p.nslots, (m >> 8) & 255) for p in by["stash"] for o, m in p.rounds if m & 3 >= 2)
    assert {(40, 0), (40, 28), (255, 243), (300, 243), (255, 0)} <= wins
    # check_at
    assert sorted(set(p.check[0] for p in by["check_at"])) == [0, 1, 2, 5, 6, 7] and all(len(p.rounds) == 6 for p in by["check_at"])
    rets = set((p.check[0], V.reference(p, "RUN_LIGHT_CHK", p.images[0])[2:]) for p in by["check_at"])
    assert {(1, (0, 1)), (1, (1, 1)), (5, (0, 1)), (5, (1, 1)), (6, (1, 0)), (7, (1, 0)), (0, (0, 1)), (0, (1, 1))} <= rets


@pytest.mark.parametrize("mutant", sorted(V.MUTANTS))
def test_every_mutant_is_told_from_tablesim(programs, mutant):
    """by some program of every class the mutant belongs to"""
    for cls in V.MUTANTS[mutant]:
        caught = [p.name for p in programs if p.cls == cls and any(not _agrees(p, op, mutant=mutant) for op in p.ops)]
        assert caught, "%s survives every program of class %s" % (mutant, cls)


def test_word_machine_is_tablesim_on_every_production_cut():
    progs, data, consts = V.production()
    ncuts = 0
    for name, op, rounds, cuts in progs:
        img = V.production_image(name, op, rounds, data, consts)
        snaps = V.production_snapshots(op, rounds, cuts, data, img)
        for c, (words, sw, res) in snaps.items():
            assert [v % Q for v in words] == res, (name, c)
            assert all(v < 2 * Q for v in words), (name, c)
            ncuts += 1
    assert ncuts > len(progs)
