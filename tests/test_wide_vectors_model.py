"""CPU: the references of tests/wide_vectors.py against each other, the static worst-case audit of every record of every table
of the wide machine, and the proof that the operand sets tell wrong arithmetic from right (one mutant of the reference executor
per way a step can be subtly wrong).  tests/test_gpu_wide.py runs the same sets on the compiled routines."""
import math

import pytest

import wide_vectors as V


@pytest.fixture(scope="module")
def ops():
    return V.ops()


def test_stored_values_and_scales():
    assert all(V.in_range(v) for v in V.STORED_INTS) and not V.in_range(V.LO - 1) and not V.in_range(V.HI + 1)
    assert 64 * (V.LO - 1) < -V.Q < 64 * V.LO and 64 * V.HI < 65 * V.Q < 64 * (V.HI + 1)      # the two ends of (-q/64, q + q/64)
    names = [n for n, _ in V.STORED]
    for n in ("lo", "hi", "zero", "q", "q-1", "one", "minus-one", "R", "R2", "ones/tmin", "ones/tmax-1", "zeros/tmax", "zeros/tmin+1"):
        assert n in names, n
    # enumerated from the models, and what the issue lists for mlw today
    assert set(V.SCALES["mlw"]) == {0, 1, -1, 2, -2, 3, -3, 6, -6, 8, -8, 12, -12, 16, -16, 24, -24, 36, -36, 72, -72}
    assert 0 in V.SRN_SCALES and set(V.SCALES["lsw"]) <= set(V.SRN_SCALES)
    assert any(2 * r.scale in V.SCALES["lsw"] for recs, h in zip(V.LW.RECS, V.LW.HAS2) if h for r in recs)


def test_per_lane_references_agree():
    for tag, t, s, ranged in V.srn_sets():
        V.check_srn(t, s, V.srn_model(t, s), ranged)
    for tag, t, s in V.scale_norm_sets():
        out = V.exec_scale_norm(t, s)
        assert all(0 <= x <= V.MASK for x in out[:-1]) and V.from_limbs(out) == s * V.from_limbs(t), tag
    zeros = 0
    for tag, d, z in V.stored_zero_sets():
        assert V.MW.is_zero_stored(d) == z, tag
        if tag != "neg-q":
            assert z == (V.from_limbs(d) % V.Q == 0), tag
        zeros += z
    assert zeros == 2                              # both digit forms of zero


def test_value_file_steps_agree_with_plain_integers():
    """every kind of every table (mlw's 35, h2cw's, g1w's) and the synthetic records: digits normalised, the residue, the stored range"""
    real, syn = V.real_wstep_sets(), V.synthetic_wstep_sets()
    kinds = set()
    for shape in V.SHAPES:
        for tag, image, rec in syn[shape] + real[shape]:
            out, _ = V.exec_wstep(image, rec, shape)
            V.check_wstep(image, rec, shape, out)
            kinds.add(tag.rsplit("/", 1)[0])
    assert len(V.MW.KINDS) == 35
    for fam, table, _ in V.TABLES:
        for step in table:
            assert "%s/%s" % (fam, step.name) in kinds
    for deg_kinds, table in ((("DBL1", "DBL2", "ADD1", "ADD2"), V.GW.KIND), (("DBL1", "DBL2", "ADD1_0p", "ADD2"), V.HW.KIND)):
        assert all(k in table for k in deg_kinds)  # both degrees of k_msm_horner_wide
    for tag, image, digs, dst, sc in V.wload_sets():
        out, _ = V.exec_wload(image, digs, dst, sc)
        assert {sc[l] * V.MW.VARIANT[l & 3] for l in range(64)} >= {3, -3, 6, -6, 1, -1, 2, -2}
        for lane in range(56):
            v = V.from_limbs(V.vf_rd(out, dst[lane]))
            assert V.in_range(v) and (v - sc[lane] * V.MW.VARIANT[lane & 3] * V.from_limbs(digs[lane])) % V.Q == 0


def test_line_stream_steps_agree_with_plain_integers():
    n = 0
    for shape, sets in V.lstep_sets().items():
        for tag, image, rec, has_line in sets:
            out, _, lines = V.exec_lstep(image, rec, shape, has_line)
            V.check_lstep(image, rec, shape, out)
            assert has_line or all(x is None for x in lines)
            n += 1
    assert n == 3 * len(V.LW.RECS) + len(V.LSHAPES) + 5 * len(V.LSHAPES)
    syn = V.synthetic_lstep_sets()
    assert all([t for t, _, _, _ in syn[sh]] == ["same-slot", "read-written", "store-order", "trash-top", "negated-operands"] for sh in V.LSHAPES)


def test_generators_refuse_a_record_past_the_bounds():
    """what replaced 'whatever s' and '<= 8': gen_mlw refuses |scale| x lanes summed past QTOP / 128, gen_lsw a column sum past 8 / 9"""
    from vmgen import gen_mlw, gen_lsw
    assert gen_mlw.SCALE_LANES_MAX == V.MW.QTOP // 128 == 832
    ok = V.MW.Step("T", [("A0", 104, [(V.MW.T((1, "X0")), V.MW.T((1, "Y0")))])])
    gen_mlw.record_words(ok)
    with pytest.raises(AssertionError):
        gen_mlw.record_words(V.MW.Step("T", [("A0", 105, [(V.MW.T((1, "X0")), V.MW.T((1, "Y0")))])]))     # 105 x 2 (the -2 multiple) x 4 lanes
    Z = V.LW.SLOT[("ZERO", 1)]
    n = [s for s in range(V.LW.NSLOTS) if s != Z and V.LSLOT_KIND[s] > 0][:2]
    full = (n[0], n[1], n[0], n[1])
    assert gen_lsw.column_units(V.LW.Rec([full] * 2, (1, 1, 1, 1), 1, None)) == (8, 0)
    with pytest.raises(AssertionError):
        gen_lsw._words(V.LW.Rec([full] * 3, (1, 1, 1, 1), 1, None), 3)
    assert max(gen_lsw.column_units(r)[0] for recs in V.LW.RECS for r in recs) == 4
    assert max(gen_lsw.column_units(r)[1] for recs in V.LW.RECS for r in recs) == 7


def test_final_exponentiation_steps_agree_with_plain_integers():
    for name, sets in V.fxw_sets().items():
        vg = "_VG" in name
        for tag, Vb, Gb, rows in sets:
            use = rows if rows is not None else V.FX_TABLES[V.FX_TABLE_OF[name]]
            assert all(abs(V.from_limbs(x)) < 2 * V.FX_MAX for x in Vb)
            V.check_fxw(Vb, Gb, use, vg, V.exec_fxw(Vb, Gb, use, vg))
    for tag, Vb, _ in V.tinv_sets():
        V.check_tinv(Vb, V.exec_tinv(Vb))
    # the fetch tables of the synthetic sets read across quads and across the 32-lane halves
    rows = dict((t, r) for t, _, _, r in V.fxw_sets()["FXW_STEP_VV"])
    assert any((rows["cross-halves"][0][l] >> 2) // 32 != l // 32 for l in range(64))
    assert any((rows["cross-quads"][0][l] >> 2) // 4 != l // 4 for l in range(64))


def test_static_audit_of_every_record(capsys):
    """worst case, not as seen: stored digits at the ends of what a slot of their kind can hold (normal: limbs in [0, 2^28), the
    value in the stored range; st14n's: limbs in (-2^28, 0]; ZERO: zero).  Each figure is measured against the hardware limit it
    guards; the figures are DESIGN.md 5's."""
    a = V.audit()
    with capsys.disabled():
        for fam, w in a.items():
            print("\naudit %-5s column units +%.3f / -%.3f (8 / 9 fit)  |top x scale| 2^%.2f (2^31)  |carry| 2^%.2f (2^63)  stored in [%.5f q, %.5f q] "
                  "((-1/64, 1 + 1/64) = (-0.01563, 1.01563))" % (fam, w["pos"], w["neg"], math.log2(w["top"]), math.log2(w["carry"]), w["lo"], w["hi"]), end="")
        print()
    for fam, w in a.items():
        assert w["pos"] <= 8 and w["neg"] <= 9, fam
        assert w["top"] < 1 << 31 and w["carry"] < 1 << 63, fam
        assert 64 * w["lo"] > -1 and 64 * w["hi"] < 65, fam
    # the worst cases themselves: the two-product steps of mlw fill the column, the line-stream formulas stay below it only because
    # of the slots they name (four products of sums of two full slots would be 16 units)
    assert a["mlw"]["pos"] > 7.99 and a["lsw"]["neg"] > 6.99


def _differs(run_ref, run_mut):
    try:
        return run_mut() != run_ref()
    except (AssertionError, IndexError):           # the mutant left int32 / int64 / the value file: it differs
        return True


MUTANT_OPS = {
    "m47+1": ("SRN",), "m47-1": ("SRN",), "quot_unscaled": ("SRN", "WSTEP_1"),
    "quad_miss_lane": ("WSTEP_2", "WSTEP_2BS", "WSTEP_1", "WSTEP_1OCT", "FXW_STEP_VV", "FXW_STEP_VG"),
    "oct_miss_quad": ("WSTEP_1OCT",), "addr_swap": ("WSTEP_2BS", "LSTEP_4", "LSTEP_2_HAS2"), "bs_adds_second": ("WSTEP_2BS",),
    "scale_zext": ("WSTEP_1", "LSTEP_3"), "st14n_carry": ("LSTEP_2", "LSTEP_4_HAS2"), "has2_reuse": ("LSTEP_2_HAS2", "LSTEP_3_HAS2", "LSTEP_4_HAS2"),
    "fxw_lane_index": ("FXW_STEP_VV", "FXW_STEP_VG"), "tinv_no_zero": ("FXW_TINV",),
}


def _caught(mut, opname):
    """the number of sets of the op on which the mutant's output differs from the reference's"""
    n = 0
    if opname == "SRN":
        return sum(_differs(lambda: V.srn_model(t, s), lambda: V._srn(t, s, mut)) for _, t, s, _ in V.srn_sets())
    if opname.startswith("WSTEP"):
        sets = V.synthetic_wstep_sets()[opname] + V.real_wstep_sets()[opname][:10]
        for tag, image, rec in sets:
            n += _differs(lambda: V.exec_wstep(image, rec, opname)[1], lambda: V.exec_wstep(image, rec, opname, mut)[1])
    elif opname.startswith("LSTEP"):
        for tag, image, rec, hl in V.lstep_sets()[opname]:
            n += _differs(lambda: V.exec_lstep(image, rec, opname, hl)[0], lambda: V.exec_lstep(image, rec, opname, hl, mut)[0])
    elif opname == "FXW_TINV":
        for tag, Vb, _ in V.tinv_sets():
            n += _differs(lambda: V.exec_tinv(Vb), lambda: V.exec_tinv(Vb, mut))
    else:
        vg = "_VG" in opname
        for tag, Vb, Gb, rows in V.fxw_sets()[opname]:
            n += _differs(lambda: V.exec_fxw(Vb, Gb, rows, vg), lambda: V.exec_fxw(Vb, Gb, rows, vg, mut))
    return n


@pytest.mark.parametrize("mut", V.MUTANTS)
def test_the_sets_catch_the_mutant(mut):
    """M47 +- 1; the quotient from the unscaled top limb; a quad sum missing a lane; the oct sum missing the other quad; the halves of
    an address word swapped; a one-slot operand that still adds its second address; the scale zero-extended; st14n with a carry
    pass; HAS2 reusing the first reduction doubled; fxw fetches by lane instead of by table; tinv without 0 -> 0"""
    assert set(MUTANT_OPS) == set(V.MUTANTS)
    for opname in MUTANT_OPS[mut]:
        assert _caught(mut, opname) >= 1, "%s: no set of %s differs" % (mut, opname)


def test_expected_words_and_layout(ops):
    """every op has sets, the expected words fit the op, only write-sink words are left out of the comparison"""
    for op in ops.values():
        assert op.sets, op.name
        for tag, words, want in op.sets:
            assert all(-(1 << 31) <= w < (1 << 31) for w in words)
            skipped = sum(x is None for x in want)
            assert skipped <= 4 * 4 * V.L, (op.name, tag, skipped)      # at most the write sink(s): never a result slot
        for n in (V.N_WAVE_ITEMS if op.wave else V.N_LANE_ITEMS):
            assert len(V.call_sets(op, n)) == n
