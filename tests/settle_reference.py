"""An independent restatement, from the Rust, of what jtk_lc_settle_nodes computes -- plain Python on run-length cigars, lists
and Python integers; nothing of the library is used.

A node is a dict(chunk, pos, fwd, qlen, cigar) with cigar = [("M" | "I" | "D", length), ...] as definitions::Op lists it: a
Match run covers mismatches.  What is restated:

    remove_slippy_alignment       haplotyper/src/encode/mod.rs:288-313
    remove_overlapping_encoding   haplotyper/src/encode/mod.rs:248-286 (the restart loop, literally)
    correct_deletion_error        haplotyper/src/encode/deletion_fill.rs:349-361 (the list surgery)
    re_encode_read                haplotyper/src/determine_chunks.rs:548-562 (the first sort by chunk alone)
    misc::max_region              haplotyper/src/misc.rs:345-358
    del_size                      haplotyper/src/purge_diverged.rs:75-80
"""
STATS_ONLY, BY_CHUNK_POS, BY_CHUNK = 0, 1, 2
UNSUPPORTED = -3
I64_MIN = -(1 << 63)


def score(cigar):
    """remove_slippy_alignment::score"""
    return sum(l if op == "M" else -l for op, l in cigar)


def total_indel(cigar):
    """the fold of remove_overlapping_encoding::start_end_iden"""
    total = indel = 0
    for op, l in cigar:
        total += l
        if op != "M":
            indel += l
    return total, indel


def max_region(xs):
    """misc::max_region: i64::MIN for an empty sequence"""
    right = left = I64_MIN
    for x in xs:
        left = max(right, left)
        right = x if right < 0 else right + x
    return max(right, left)


def div_toward_zero(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def del_size(cigar):
    """purge_diverged.rs:75-80 with DEL_WEIGHT 2, MATCH_WEIGHT 1"""
    return div_toward_zero(max_region(-l if op == "M" else 2 * l for op, l in cigar), 2)


def query_bases(cigar):
    return sum(l for op, l in cigar if op != "D")


def node_stats(node):
    """(score, total, indel, del_size); a node without ops has no del_size in the reference: all four are 0 here"""
    cigar = node["cigar"]
    if not cigar:
        return (0, 0, 0, 0)
    total, indel = total_indel(cigar)
    return (score(cigar), total, indel, del_size(cigar))


def remove_slippy_alignment(nodes):
    deduped = []
    it = iter(nodes)
    prev = next(it)
    for node in it:
        is_disjoint = prev["pos"] + prev["qlen"] < node["pos"]
        if prev["chunk"] != node["chunk"] or prev["fwd"] != node["fwd"] or is_disjoint:
            deduped.append(prev)
            prev = node
        elif score(prev["cigar"]) < score(node["cigar"]):
            prev = node
    deduped.append(prev)
    return deduped


def start_end_iden(node):
    total, indel = total_indel(node["cigar"])
    return node["pos"], node["pos"] + node["qlen"], 1.0 - float(indel) / float(total)


def remove_overlapping_encoding(nodes):
    nodes = list(nodes)
    while True:
        should_be_removed = None
        for i in range(len(nodes) - 1):
            fs, fe, fi = start_end_iden(nodes[i])
            ls, le, li = start_end_iden(nodes[i + 1])
            if (fs <= ls and le < fe) or (ls <= fs and fe < le):
                should_be_removed = i if fi < li else i + 1
                break
        if should_be_removed is None:
            return nodes
        del nodes[should_be_removed]


def settle_read(nodes, mode):
    """the indices into `nodes` that survive, in their final order"""
    tagged = [dict(n, idx=i) for i, n in enumerate(nodes)]
    if mode == BY_CHUNK_POS:
        tagged.sort(key=lambda n: (n["chunk"], n["pos"]))      # list.sort is stable, as sort_by_key is
    else:
        tagged.sort(key=lambda n: n["chunk"])
    tagged = remove_slippy_alignment(tagged)
    tagged.sort(key=lambda n: n["pos"])
    tagged = remove_slippy_alignment(tagged)
    tagged = remove_overlapping_encoding(tagged)
    return [n["idx"] for n in tagged]


def settle(reads, mode):
    """reads: a list of node lists.  Returns dict(stats, keep, order, n_kept, status, rc): stats and keep per node in input
    order (flat), order per read, status per read (UNSUPPORTED where a node has no ops or its cigar does not take qlen bases:
    the read is left as it came), rc = -6 where a read has a status."""
    stats, keep, order, n_kept, status = [], [], [], [], []
    for nodes in reads:
        stats += [node_stats(n) for n in nodes]
        bad = any(not n["cigar"] or query_bases(n["cigar"]) != n["qlen"] for n in nodes)
        status.append(UNSUPPORTED if bad else 0)
        if bad or mode == STATS_ONLY or not nodes:
            kept = list(range(len(nodes)))
        else:
            kept = settle_read(nodes, mode)
        order.append(kept)
        n_kept.append(len(kept))
        keep += [1 if i in kept else 0 for i in range(len(nodes))]
    return dict(stats=stats, keep=keep, order=order, n_kept=n_kept, status=status, rc=-6 if any(status) else 0)


def per_base(cigar):
    """the ABI's per-base ops of a cigar: Match 0 (every third base of a Match run is written as Mismatch 1, which the cigar
    does not tell apart), Ins 2, Del 3"""
    out = []
    for op, l in cigar:
        if op == "M":
            out += [1 if i % 3 == 2 else 0 for i in range(l)]
        else:
            out += [2 if op == "I" else 3] * l
    return out


def per_base_del_size(ops):
    """the statement of include/jtk_lc.h on per-base ops: the largest sum of a non-empty range of the weights (-1 Match or
    Mismatch, +2 Ins or Del), halved toward zero, where the node has an indel; -(total) / 2 toward zero where it has none"""
    if not any(o >= 2 for o in ops):
        return div_toward_zero(-len(ops), 2)
    best = None
    for i in range(len(ops)):
        s = 0
        for j in range(i, len(ops)):
            s += 2 if ops[j] >= 2 else -1
            best = s if best is None or s > best else best
    return div_toward_zero(best, 2)
