"""The host side of a pairing call stated on its own: which Miller kernel runs, the partials per group, chunks and merge levels of
the line-stream stage, the levels of the reduce chain, the form of the final exponentiation, the buffer sizes and the slices.
Written from csrc/blsgpu_api.hip as it stood at commit 671d860 ("Check the hash-to-curve register layer on the device, word for
word"), BEFORE csrc/pairing_plan.h existed -- use_mp .. ensure_partials, launch_fexp_* .. blsgpu_pairing_multi_batch_dev and
blsgpu_ctx_reserve, where this arithmetic stood inline between the launches -- so that the header is held against what the
library did, not against itself (tests/test_pairing_plan_host.py).

Every function returns the list of numbers the host test's program prints for the same plan.  The slice lengths, literals in that
commit (32768 groups, 1 << 20 pairs of line records, 262144 exact pairs), are the argument L."""
import errno

# the kernel files' constants (blsgpu_ml.hip, blsgpu_kernels.hip, vm_tables.h, fexp_tables_gfx950.h) and blsgpu_api.hip's own
NL = 14
LINES, LINE_DW, DENSE_DW, TEAMS, SLAB_BYTES_PER_LANE = 68, 6 * NL, 12 * NL, 10, 4 * NL * 4
MP_G, TEAM_BYTES, MP_TEAM_BYTES, SLOW_TEAM_BYTES, FEXP_NSLOTS = 3, 212 * 48, 212 * 48, 212 * 48, 5
MILLER_WAVES, REDUCE_WAVES, REDUCE_PER_BLOCK, BATCH_TREE_MIN_GROUP, FAN, SLOW_GRID = 4, 8, 64, 24, 8, 3072
CONSTS = [LINES, LINE_DW, DENSE_DW, TEAMS, SLAB_BYTES_PER_LANE, MP_G, TEAM_BYTES, MP_TEAM_BYTES, SLOW_TEAM_BYTES, FEXP_NSLOTS,
          MILLER_WAVES, REDUCE_WAVES, REDUCE_PER_BLOCK, BATCH_TREE_MIN_GROUP, FAN, SLOW_GRID]
LITERALS = (32768, 1 << 20, 262144)                          # max_groups, ls_max_pairs, exact_slice

NEVER = (1 << 64) - 1                                        # (size_t)-1
# the knobs, in the order the host test passes them, with the defaults of blsgpu_ctx
KNOBS = dict(miller_wide3_max=256, miller_wide_max=1536, mp_threshold=4096, mp3_threshold=NEVER, ls_threshold=2304, ls_min_group=64,
             ls_teams=163840, ls_merge_wide_max=16384, ls_wide_max=5120, ls_quad_max=20480, fexp_team_threshold=5120, fexp_wide=1,
             fexp_wide_max_partials=8, vm_exact_lanes=1, miller_exact_lanes=1, miller_exact_fast=1, test_ls_nomem=0)

FEXP_NONE, FEXP_TEAM, FEXP_WIDE = range(3)
M_WIDE3, M_WIDE2, M_MP2, M_MP3, M_VM = range(5)
OK, BATCH_TOO_LARGE, PARTIALS_TOO_SMALL, WORK_LIST_TOO_SMALL, TOO_MANY_GROUPS, WORKSPACE_TOO_SMALL = range(6)
REFUSALS = {OK: (0, ""), BATCH_TOO_LARGE: (-errno.EINVAL, "batch too large"),
            PARTIALS_TOO_SMALL: (-errno.ENOMEM, "partial buffer too small for the Miller kernel's blocks"),
            WORK_LIST_TOO_SMALL: (-errno.ENOMEM, "work list too small"), TOO_MANY_GROUPS: (-errno.EINVAL, "too many groups"),
            WORKSPACE_TOO_SMALL: (-errno.ENOMEM, "workspace too small; call blsgpu_ctx_reserve")}
L_WIDE16, L_QUAD, L_PAIR = range(3)
RB_IN, RB_PART0, RB_PART1, RB_OUT = range(4)
R_REG, R_HAND_OVER, R_REDUCE = range(3)
LS_OFF, LS_WHOLE, LS_GROUP_SLICES, LS_RUN_SLICES, LS_VM_LONG_GROUPS = range(5)
B_TREE, B_LS_SMALL, B_TEAM_GROUPS, B_ONE_PER_BLOCK = range(4)


def knobs(**over):
    assert set(over) <= set(KNOBS)
    return dict(KNOBS, **over)


def cdiv(a, b):
    return -(-a // b)


def use_mp(c, n):
    return n >= c["mp_threshold"]


def use_mp2(c, n):
    if c["mp3_threshold"] != NEVER:
        return n < c["mp3_threshold"]
    return n <= 8704 or 9728 < n <= 11264 or 14336 < n <= 18432


def pairs_partials(pairs):
    return (pairs + 1) // 2 + cdiv(pairs, MILLER_WAVES) + 1


def use_fexp_team(c, m, groups):
    return groups >= c["fexp_team_threshold"] and m <= 64


def use_fexp_wide(c, m, groups):
    return bool(c["fexp_wide"]) and groups < c["fexp_team_threshold"] and 1 <= m <= c["fexp_wide_max_partials"] and groups <= 0x7FFFFFFF


def use_fexp_reg(c, m, groups):
    return use_fexp_team(c, m, groups) or use_fexp_wide(c, m, groups)


def fexp_form(c, m, groups):
    """launch_fexp_reg: [kind, wavefronts asked of wave_shape, bytes of B_FEXP_WS per launched wavefront]"""
    if use_fexp_team(c, m, groups):
        return [FEXP_TEAM, cdiv(groups, TEAMS), (TEAMS + 1) * FEXP_NSLOTS * DENSE_DW * 4]
    return [FEXP_WIDE if use_fexp_wide(c, m, groups) else FEXP_NONE, 0, 0]


def miller(c, gsz, groups, one_per_block, team, own, part_cap, degen_cap):
    """miller_plan + launch_miller"""
    n = gsz * groups
    wide = not team and n <= c["miller_wide_max"] and not use_mp(c, n)
    mp = True if team else (not wide and not one_per_block and use_mp(c, n))
    mp2 = team == 2 if team else (mp and use_mp2(c, n))
    per_block = 1 if (one_per_block or wide) else ((2 if mp2 else MP_G) if mp else MILLER_WAVES)
    bpg = cdiv(gsz, per_block)
    blocks = bpg * groups
    if wide:
        kernel = M_WIDE3 if n <= c["miller_wide3_max"] else M_WIDE2
    else:
        kernel = M_MP2 if mp2 else M_MP3 if mp else M_VM
    head = [kernel, per_block, bpg, blocks, n]
    if blocks > 0x7FFFFFFF:
        return head + [BATCH_TOO_LARGE]
    if own and blocks > part_cap:
        return head + [PARTIALS_TOO_SMALL]
    if blocks + 2 > degen_cap:
        return head + [WORK_LIST_TOO_SMALL]
    grid, threads, lds = {M_WIDE3: (blocks, 192, 0), M_WIDE2: ((blocks + 1) // 2, 256, 0), M_MP2: (blocks, 64, MP_TEAM_BYTES),
                          M_MP3: (blocks, 64, MP_TEAM_BYTES), M_VM: (blocks, per_block * 64, per_block * TEAM_BYTES)}[kernel]
    nv = blocks * per_block
    exact = int(bool(c["vm_exact_lanes"]) and nv <= 1 << 16)
    tail = [nv * LINES * LINE_DW * 4, nv, cdiv(blocks, TEAMS)] if exact else [0, 0, 0]
    return head + [OK, grid, threads, lds, nv, exact] + tail


def use_ls(c, gsz, groups):
    return gsz >= 1 and c["ls_threshold"] <= gsz * groups <= 0x3FFFFFF0


def ls(c, gsz, groups, one_per_group, want_fused):
    """launch_miller_ls"""
    n = gsz * groups
    aim = n * LINES // 128
    aim = max(aim, 40960)
    aim = min(aim, c["ls_teams"])
    want = cdiv(n * LINES, aim)
    want = max(want, 16)
    want = min(want, gsz)
    cpg = cdiv(gsz, want)
    chunk = cdiv(gsz, cpg)
    cpg = cdiv(gsz, chunk)
    small = int(one_per_group or gsz < c["ls_min_group"])
    lsp0 = 0 if small else groups * cpg * LINES * DENSE_DW * 4
    lsp1 = 0 if small else groups * cdiv(cpg, FAN) * LINES * DENSE_DW * 4
    if n <= c["ls_wide_max"]:
        chain, waves = L_WIDE16, (2 * n + 63) // 64
    elif n <= c["ls_quad_max"]:
        chain, waves = L_QUAD, (4 * n + 63) // 64
    else:
        chain, waves = L_PAIR, (2 * n + 63) // 64
    out = [n, chunk, cpg, small, n * LINES * LINE_DW * 4, lsp0, lsp1, n, (n + 2) * 4, chain, cdiv(n, 16), waves, cdiv(groups, TEAMS)]
    if small:
        return out + [0, 0, 0, 0, 0]
    teams = groups * cpg * LINES
    out += [teams, cdiv(teams, TEAMS)]
    cur, levels = 0, []
    while cpg > 1:
        cpo = cdiv(cpg, FAN)
        teams = groups * cpo * LINES
        levels += [cpg, cpo, teams, cdiv(teams, TEAMS), int(teams <= c["ls_merge_wide_max"]), cur, cur ^ 1]
        cpg = cpo
        cur ^= 1
    fuse = int(bool(want_fused) and use_fexp_wide(c, 1, groups))
    return out + [len(levels) // 7] + levels + [cur, fuse]


def reduce(c, m, groups, istride, gstride, do_final, from_part0, part_cap):
    """reduce_chain: [refusal] or [OK, levels ..., end, form of the final exponentiation, what it reads]"""
    if groups > 65535:
        return [TOO_MANY_GROUPS]
    src = RB_PART0 if from_part0 else RB_IN
    pp = 1 if from_part0 else 0
    levels = []

    def done(end, form, fsrc, fm, fi, fg):
        return [OK, len(levels) // 7] + levels + [end] + form + [fsrc, fm, fi, fg, REDUCE_WAVES * TEAM_BYTES]
    while True:
        if do_final and use_fexp_reg(c, m, groups):
            return done(R_REG, fexp_form(c, m, groups), src, m, istride, gstride)
        blocks = cdiv(m, REDUCE_PER_BLOCK) or 1
        last = blocks == 1
        hand_over = last and do_final and use_fexp_reg(c, 1, groups) and groups <= part_cap
        dst = RB_OUT if (last and not hand_over) else (RB_PART1 if pp else RB_PART0)
        if not last and blocks * groups > part_cap:
            return [WORKSPACE_TOO_SMALL]
        fin = int(bool(last and do_final and not hand_over))
        levels += [blocks, m, istride, gstride, dst, fin, 2 if fin else 1]
        if hand_over:
            return done(R_HAND_OVER, fexp_form(c, 1, groups), dst, 1, 1, 1)
        if last:
            return done(R_REDUCE, [FEXP_NONE, 0, 0], RB_IN, 0, 0, 0)
        src, m, istride, gstride, pp = dst, blocks, 1, blocks, pp ^ 1


def grouped(c, L, gsz, groups, want_bytes, want_partial):
    """grouped_pairing: [outer, partials, mode, per, runs, run length, direct, bpg after the line-stream stage, bpg of the VM kernels]"""
    max_groups, ls_max_pairs, _ = L
    if groups > max_groups:
        return [max_groups, 0, 0, 0, 0, 0, 0, 0, 0]
    partials = pairs_partials((gsz + 3) * groups)
    vm_bpg = miller(c, gsz, groups, False, 0, False, 0, NEVER)[2] if gsz else 0
    partials = max(partials, vm_bpg * groups)
    mode = per = runs = run_len = direct = ls_bpg = 0
    if gsz > 0 and use_ls(c, gsz, groups):
        ls_bpg = 1
        if gsz * groups <= ls_max_pairs:
            mode, direct = LS_WHOLE, int(bool(want_partial and not want_bytes))
        elif gsz <= ls_max_pairs:
            mode, per = LS_GROUP_SLICES, ls_max_pairs // gsz
        elif groups == 1:
            mode, run_len = LS_RUN_SLICES, ls_max_pairs
            ls_bpg = runs = len(range(0, gsz, ls_max_pairs))
        else:
            mode, ls_bpg = LS_VM_LONG_GROUPS, 0
    return [0, partials, mode, per, runs, run_len, direct, ls_bpg, vm_bpg]


def batch(c, L, gsz, groups):
    """blsgpu_pairing_multi_batch_dev: [route, route without the line-stream workspace, partials, n, final stage of each]"""
    n = gsz * groups
    if gsz >= BATCH_TREE_MIN_GROUP:
        return [B_TREE, B_TREE, 0, n] + [0] * 14
    partials = 3 * (n + 1) + 1
    team_groups = (gsz == 2 or gsz == MP_G) and use_mp(c, n) and groups <= 0x7FFFFFFF
    fallback = B_TEAM_GROUPS if team_groups else B_ONE_PER_BLOCK
    route = B_LS_SMALL if (gsz >= 1 and use_ls(c, gsz, groups) and n <= L[1]) else fallback

    def final(r):
        m = gsz if r == B_ONE_PER_BLOCK else 1
        return [m, 1, m] + fexp_form(c, m, groups) + [cdiv(groups, REDUCE_WAVES)]
    return [route, fallback, partials, n] + final(route) + final(fallback)


def exact(L, n):
    """blsgpu_miller_loop_batch_dev: the sizes, then every slice"""
    step = L[2]
    m0 = min(n, step)
    out = [n, step, m0, m0 + (m0 + 1) // 2 + 1, 2 * m0, m0 * LINES * LINE_DW * 4, m0, (m0 + 2) * 4, min(n, 16384)]
    los = list(range(0, n, step))
    if len(los) > 8:
        los = los[:4] + los[-3:]
    out.append(len(los))
    for lo in los:
        m = min(n - lo, step)
        out += [lo, m, cdiv(m, 256), cdiv(2 * m, 256), cdiv(m, 256), cdiv(m * 12, 256), cdiv(m, TEAMS)]
    return out


def reserve(c, L, max_pairs):
    """blsgpu_ctx_reserve"""
    if max_pairs < c["ls_threshold"]:
        return [pairs_partials(max_pairs), 0, 0, 0, 0, 0, 0]
    n = min(max_pairs, L[1])
    teams = c["ls_teams"] + LINES * (n // (c["ls_min_group"] or 1) + 1)
    return [pairs_partials(max_pairs), 1, n * LINES * LINE_DW * 4, n, (n + 2) * 4, teams * DENSE_DW * 4, (teams // 8 + LINES) * DENSE_DW * 4]


def lines(c, L, part_cap, gsz, groups):
    """the lines the host test's program prints for a case"""
    def line(name, v):
        return " ".join([name] + [str(int(x)) for x in v])
    n = gsz * groups
    out = [line("fexp", fexp_form(c, gsz, groups) + fexp_form(c, 1, groups))]
    for opb, team in [(0, 0), (1, 0)] + ([(0, gsz)] if gsz in (2, MP_G) else []):
        out.append(line("miller", miller(c, gsz, groups, opb, team, not opb, part_cap, part_cap + 2)))
    if gsz >= 1 and n <= 0x3FFFFFF0:
        out.append(line("ls", ls(c, gsz, groups, False, True)))
        out.append(line("ls", ls(c, gsz, groups, True, False)))
    for args in [(gsz, groups, 1, gsz, 1, 1), (gsz, groups, 1, gsz, 0, 1), (gsz, groups, groups, 1, 1, 0)]:
        out.append(line("reduce", reduce(c, *args, part_cap)))
    out.append(line("grouped", grouped(c, L, gsz, groups, 1, 0)))
    out.append(line("grouped", grouped(c, L, gsz, groups, 0, 1)))
    out.append(line("batch", batch(c, L, gsz, groups)))
    out.append(line("exact", exact(L, gsz)))
    out.append(line("reserve", reserve(c, L, gsz)))
    return out
