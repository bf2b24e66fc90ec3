"""An independent restatement of the candidate search of correct_deletion (haplotyper/src/encode/deletion_fill.rs:611-1136, and
the threshold of :312-314): check_alignment_by_chunkmatch, pairwise_alignment_gotoh with its traceback, `alignment`'s verdict,
get_pileup's walk, Pileup::check_insertion_head / _tail.  Plain Python ints; every DP value is asserted to lie in int32.  It is
written from the reference alone and shares no code with the device implementation.

A read is a list of nodes (chunk, cluster, is_forward, query_len, position).  A light node is the tuple
(chunk, cluster, is_forward, prev_offset, after_offset) with None for an absent offset."""

MIN_ALN = -10000000
MIN_MATCH = 2
SCORE_THR = 1
INS_THR = 2
INT32 = (-(1 << 31), (1 << 31) - 1)
MATCH, INS, DEL = 0, 1, 2     # op codes of the compressed ops, as (code, length)


# ---- the three rules that are easy to get wrong, by name

def last_max(items, key):
    """Iterator::max_by_key: the LAST element among the maximal ones."""
    best = None
    for it in items:
        if best is None or key(it) >= key(best):
            best = it
    return best


def first_equal(values, wanted):
    """Iterator::find over an enumerate: the index of the FIRST value equal to `wanted`."""
    for i, v in enumerate(values):
        if v == wanted:
            return i
    raise AssertionError("no predecessor state carries the value")


def div_trunc(a, b):
    """isize / isize: the quotient rounded toward zero."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def as_isize(x):
    """`as isize` of a u64 / the wrap of an isize sum."""
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


def in_i32(v):
    assert INT32[0] <= v <= INT32[1], v
    return v


# ---- ReadSkelton :999-1035, LightNode :1080-1100

def skeleton(nodes):
    spans = [(as_isize(p), as_isize(p + q)) for (_, _, _, q, p) in nodes]
    out = []
    for i, (chunk, cluster, fwd, _, _) in enumerate(nodes):
        prev = as_isize(spans[i][0] - spans[i - 1][1]) if i > 0 else None
        after = as_isize(spans[i + 1][0] - spans[i][1]) if i + 1 < len(nodes) else None
        out.append((chunk, cluster, bool(fwd), prev, after))
    return out


def key(n):
    return (n[0], n[1], n[2])


def rev_node(n):
    return (n[0], n[1], not n[2], n[4], n[3])


def rev(skel):
    return [rev_node(n) for n in reversed(skel)]


# ---- check_alignment_by_chunkmatch :611-637

def count_match(a, b):
    i = j = num = 0
    while i < len(a) and j < len(b):
        if a[i] < b[j]:
            i += 1
        elif a[i] == b[j]:
            num += 1
            i += 1
            j += 1
        else:
            j += 1
    return num


def chunkmatch(sorted_target_keys, query):
    """None (no alignment is tried), or the direction: True = forward."""
    keys = sorted(key(n) for n in query)
    forward = count_match(sorted_target_keys, keys)
    keys = sorted((c, k, not f) for (c, k, f) in keys)
    reverse = count_match(sorted_target_keys, keys)
    min_match = min(MIN_MATCH, len(sorted_target_keys))
    if min_match <= max(forward, reverse):
        return reverse <= forward
    return None


# ---- pairwise_alignment_gotoh :738-827

def score(x, y):
    if x[0] != y[0] or x[2] != y[2]:
        return MIN_ALN
    return 1 if x[1] == y[1] else -1


def gotoh(read, query):
    """(score, compressed ops) of `read` (rows) against `query` (columns)."""
    n, m = len(read), len(query)
    dp = [[[0, 0, 0] for _ in range(m + 1)] for _ in range(n + 1)]
    for i in range(n + 1):
        dp[i][0][0] = MIN_ALN
        dp[i][0][1] = MIN_ALN
    for j in range(m + 1):
        dp[0][j][0] = MIN_ALN
        dp[0][j][2] = MIN_ALN
    dp[0][0][0] = 0
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            cell = dp[i][j]
            cell[0] = in_i32(max(dp[i - 1][j - 1]) + score(read[i - 1], query[j - 1]))
            cell[1] = in_i32(max(dp[i][j - 1][0] - 1, dp[i][j - 1][1]))
            cell[2] = in_i32(max(dp[i - 1][j][0] - 1, dp[i - 1][j][2]))
    ends = [(i, m) for i in range(n + 1)] + [(n, j) for j in range(m + 1)]
    cells = []
    for (i, j) in ends:
        state, value = last_max(list(enumerate(dp[i][j])), key=lambda sv: sv[1])
        cells.append((i, j, state, value))
    r, q, state, dist = last_max(cells, key=lambda c: c[3])
    ops = []
    if n != r:
        ops.append((DEL, n - r))
    if m != q:
        ops.append((INS, m - q))
    while r > 0 and q > 0:
        cur = dp[r][q][state]
        if state == 0:
            state = first_equal(dp[r - 1][q - 1], cur - score(read[r - 1], query[q - 1]))
            ops.append((MATCH, 1))
            r -= 1
            q -= 1
        elif state == 1:
            state = int(cur != dp[r][q - 1][0] - 1)
            ops.append((INS, 1))
            q -= 1
        else:
            state = 0 if cur == dp[r - 1][q][0] - 1 else 2
            ops.append((DEL, 1))
            r -= 1
    assert r == 0 or q == 0
    if r != 0:
        ops.append((DEL, r))
    if q != 0:
        ops.append((INS, q))
    ops.reverse()
    return dist, compress(ops)


def compress(ops):
    assert ops
    out = []
    cur = ops[0]
    for op in ops[1:]:
        if op[0] == cur[0]:
            cur = (cur[0], cur[1] + op[1])
        else:
            out.append(cur)
            cur = op
    out.append(cur)
    return out


def is_proper(ops):
    return all({a[0], b[0]} != {INS, DEL} for a, b in zip(ops, ops[1:]))


def alignment(read, query, forward):
    """(score, ops, passed) -- `alignment` :707-719 returns the ops only where `passed`."""
    dist, ops = gotoh(read, query if forward else rev(query))
    matched = sum(l for (c, l) in ops if c == MATCH)
    min_match = min(MIN_MATCH, len(read), len(query))
    return dist, ops, (min_match <= matched and SCORE_THR <= dist and is_proper(ops))


def pair(read_nodes, query_nodes):
    """What jtk_lc_debug_fill_pairs reports of one (target, query) pair: direction (1 forward, 0 reverse, -1 = the pre-filter
    rejects the pair, nothing else is computed), score, pass flag, compressed ops."""
    read, query = skeleton(read_nodes), skeleton(query_nodes)
    forward = chunkmatch(sorted(key(n) for n in read), query) if read else None    # a read without nodes is never a target
    if forward is None:
        return {"dir": -1, "score": 0, "pass": 0, "ops": []}
    dist, ops, ok = alignment(read, query, forward)
    return {"dir": int(forward), "score": dist, "pass": int(ok), "ops": ops}


# ---- get_pileup :642-698

class SkeltonIter:
    def __init__(self, skel, forward):
        self.skel, self.forward = skel, forward
        self.index = 0 if forward else len(skel)

    def next(self):
        if self.forward:
            self.index += 1
            return self.skel[self.index - 1] if self.index - 1 < len(self.skel) else None
        if self.index > 0:
            self.index -= 1
            return rev_node(self.skel[self.index])
        return None

    def nth(self, k):
        for _ in range(k):
            self.next()
        return self.next()


def get_pileup(read, skeletons):
    """[coverage, head list, tail list] per slot 0 ..= n."""
    n = len(read)
    assert n > 0
    pile = [[0, [], []] for _ in range(n + 1)]
    keys = sorted(key(x) for x in read)
    for query in skeletons:
        forward = chunkmatch(keys, query)
        if forward is None:
            continue
        _, ops, ok = alignment(read, query, forward)
        if not ok:
            continue
        it = SkeltonIter(query, forward)
        taken = 1            # the shadowing iter_mut() has yielded slot 0: `taken` slots are gone, n + 1 - taken remain
        cur = 0
        position = 0
        for (code, l) in ops:
            remaining_minus_1 = (n + 1 - taken - 1) & ((1 << 64) - 1)     # pileups.len() - 1, wrapping (release build)
            if code == INS and position == 0:
                pile[cur][2].append(it.nth(l - 1))
            elif code == INS and position == remaining_minus_1:
                pile[cur][1].append(it.next())
                for _ in range(l - 1):
                    assert it.next() is not None
            elif code == INS:
                pile[cur][1].append(it.next())
                if 2 <= l:
                    pile[cur][2].append(it.nth(l - 2))
            elif code == DEL:
                taken += l
                cur = taken - 1
                assert cur <= n
                position += l
            else:
                it.nth(l - 1)
                position += l
                for _ in range(l):
                    pile[cur][0] += 1
                    taken += 1
                    cur = taken - 1
                    assert cur <= n
            assert cur == position
        for slot in pile:
            assert None not in slot[1] and None not in slot[2]
    return pile


# ---- Pileup::check_insertion_head / _tail :883-981

def summarize(inserts, which):
    """key -> (entries, truncated mean of the present offsets or None); which = 3 (prev_offset) or 4 (after_offset)."""
    out = {}
    for n in inserts:
        cnt, present, total = out.get(key(n), (0, 0, 0))
        if n[which] is not None:
            present, total = present + 1, total + n[which]
        out[key(n)] = (cnt + 1, present, total)
    return {k: (cnt, div_trunc(total, present) if present else None) for k, (cnt, present, total) in out.items()}


def candidates_of_read(r, nodes, pile, ins_thr):
    n = len(nodes)
    out = []
    for slot in range(n + 1):
        head = summarize(pile[slot][1], 3)
        if slot == 0:
            assert not head      # an insertion at position 0 only ever goes to the tail list
        for k, (cnt, off) in head.items():
            if ins_thr <= cnt and off is not None:
                start = nodes[slot - 1][4] + nodes[slot - 1][3]
                out.append((r, slot, 0, k[0], k[1], int(k[2]), cnt, as_isize(as_isize(start) + off)))
        if slot < n:
            for k, (cnt, off) in summarize(pile[slot][2], 4).items():
                if ins_thr <= cnt and off is not None:
                    out.append((r, slot, 1, k[0], k[1], int(k[2]), cnt, max(as_isize(nodes[slot][4]) - off, 0)))
    return sorted(out, key=lambda c: c[:6])


def fill_candidates(reads, target=None):
    """reads: list of node lists.  Returns coverage (flat, read r's n + 1 slots at node_off[r] + r), ins_thr, cand_off and
    cands as tuples (read, slot, side, chunk, cluster, is_forward, count, position) in the order of the interface.  A read that
    is no target (or has no node) keeps zero coverage, ins_thr 0 and no candidate."""
    skels = [skeleton(r) for r in reads]
    coverage, ins_thr, cand_off, cands = [], [], [0], []
    for r, nodes in enumerate(reads):
        n = len(nodes)
        if n == 0 or (target is not None and not target[r]):
            coverage += [0] * (n + 1)
            ins_thr.append(0)
            cand_off.append(len(cands))
            continue
        pile = get_pileup(skels[r], skels)
        cov = [p[0] for p in pile]
        assert cov[n] == 0
        thr = min((sum(cov) // (n + 1)) // 5, INS_THR)
        coverage += cov
        ins_thr.append(thr)
        cands += candidates_of_read(r, nodes, pile, thr)
        cand_off.append(len(cands))
    return {"coverage": coverage, "ins_thr": ins_thr, "cand_off": cand_off, "cands": cands}
