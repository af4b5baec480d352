"""The plan of the three bisecting checks (blsgpu_verify_find, blsgpu_verify_find_folded, blsgpu_sig_shares_check) stated on its
own, from what their documentation promises, with the verdict rule "a node fails iff it holds a forged leaf":

  * the leaves 0 .. limit - 1 are tested in aligned nodes (offset, length), all nodes of a round of one length, the first round
    one node of the length `limit` rounded up to a power of two; a node ends at min(offset + length, limit);
  * a node that failed is replaced, where it stood, by its first half and -- if that begins before `limit` -- its second half;
    the rounds end after the leaves, or when nothing failed;
  * plain: the nodes that end at offset + length come first, then the one cut short by the limit; a node of `len` leaves feeds
    len + 1 pairs;
  * folded: a node feeds one pair and one more per message among its leaves (the leaves are sorted by message); the nodes of a
    round are ordered by their pair count, the earlier order kept among equals;
  * shares: every session is bisected over its k shares, all sessions side by side, a round for every length some session needs.

Each function returns {"named": the leaves found forged, "stats": what the call reports, "rounds": [(length, nodes in order)]}."""


def ceil_pow2(n):
    return 1 << (n - 1).bit_length() if n > 1 else 1


def layout(unit, start, counts):
    """offsets of consecutive arrays, each rounded up to a multiple of `unit`; -> (offsets, end)"""
    offs = []
    for c in counts:
        offs.append(start)
        start += -(-c // unit) * unit
    return offs, start


def run_table_ok(n_e, n_runs, cap, rb):
    """runs 0 .. n_runs - 1 tile [0, n_e) and fit the `cap` entries of the table"""
    return 0 < n_runs < cap and rb[0] == 0 and rb[n_runs] == n_e


def _bisect(limit, forged, arrange, fed):
    """`arrange(nodes, length)`: the nodes in the order of the round; `fed(off, end)`: the pairs of a node"""
    length = ceil_pow2(limit)
    nodes, rounds, tests, pairs, named = [0], [], 0, 0, set()
    while nodes:
        nodes = arrange(nodes, length)
        ends = [min(o + length, limit) for o in nodes]
        rounds.append((length, list(nodes)))
        tests += len(nodes)
        pairs += sum(fed(o, e) for o, e in zip(nodes, ends))
        failed = [o for o, e in zip(nodes, ends) if any(o <= f < e for f in forged)]
        if length == 1:
            named.update(failed)
            break
        length //= 2
        nodes = [h for o in failed for h in (o, o + length) if h < limit]
    return {"named": named, "stats": (len(rounds), tests, pairs), "rounds": rounds}


def plain(n_e, forged):
    def arrange(nodes, length):
        return [o for o in nodes if o + length <= n_e] + [o for o in nodes if o + length > n_e]
    return _bisect(n_e, forged, arrange, lambda o, e: e - o + 1)


def pair_ranges(msgs, off, end):
    """the (message, lo, hi) of the leaves off .. end - 1, one per message"""
    out = []
    for i in range(off, end):
        if out and out[-1][0] == msgs[i]:
            out[-1][2] = i + 1
        else:
            out.append([msgs[i], i, i + 1])
    return [tuple(r) for r in out]


def folded(msgs, forged):
    """msgs: the message of every leaf, non-decreasing"""
    n_e = len(msgs)

    def fed(o, e):
        return 1 + len(pair_ranges(msgs, o, e))

    def arrange(nodes, length):
        return sorted(nodes, key=lambda o: fed(o, min(o + length, n_e)))     # sorted() is stable
    return _bisect(n_e, forged, arrange, fed)


def shares(k, forged):
    """forged: per session the set of its forged shares"""
    per = [_bisect(k, f, lambda nodes, length: nodes, lambda o, e: 0) for f in forged]
    rounds = []
    for lv in range(max(len(p["rounds"]) for p in per)):
        length = ceil_pow2(k) >> lv
        rounds.append((length, [(s, o) for s, p in enumerate(per) if lv < len(p["rounds"]) for o in p["rounds"][lv][1]]))
    return {"named": [p["named"] for p in per], "stats": (len(rounds), sum(p["stats"][1] for p in per)), "rounds": rounds}


def runs_of(msgs):
    """the run table of a sorted list of messages: (rb, rmsg), run r = leaves rb[r] .. rb[r + 1] - 1 of message rmsg[r]"""
    r = pair_ranges(msgs, 0, len(msgs))
    return [lo for _, lo, _ in r] + [len(msgs)], [m for m, _, _ in r]
