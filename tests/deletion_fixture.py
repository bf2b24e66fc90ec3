"""The planted data set of tests/test_gpu_correct_deletion.py, tests/test_deletion_driver.py and scripts/settle_timing.py: a JTK
`DataSet` as parsed from JSON with 12 reads (3 of them reverse) over 5 chunks of 200 bases, simulated with one error profile at
a fixed seed; the middle node is taken out of 3 reads, one of those reads also carries a second, shifted node of chunk 1, 4 reads
lack 60 bases of chunk 3, and chunk 1 has a second cluster of 5 nodes."""
import copy
import functools

import numpy as np

import align_reference as AR
import deletion_reference as DR
import purge_reference as PR

CHUNK_LEN, SPACER, N_CHUNKS, N_READS = 200, 50, 5, 12
MISSING = (2, 5, 8)          # reads without their node of chunk 2
DUPLICATE = 5                # ... of which this one carries a second node of chunk 1
DELETED = (0, 3, 6, 9)       # reads that lack 60 bases of chunk 3
REVERSE = (1, 5, 10)
SECOND = (0, 4, 7, 8, 11)    # reads whose node of chunk 1 is in that chunk's second cluster (its consensus is polished)
SMALL_INDEL = 30             # the indel_size at which purge_largeindel fires on this fixture
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def simulate(rng, genome, holes, rate=0.03):
    """the genome with substitutions, insertions and deletions at `rate` and without the positions in `holes`
    -> (read, where each genome position starts in the read)"""
    out, at = [], []
    for g, base in enumerate(genome):
        at.append(len(out))
        if g in holes:
            continue
        u = rng.random()
        if u < rate / 3:
            out.append(int(rng.choice([b for b in b"ACGT" if b != base])))
        elif u < 2 * rate / 3:
            continue
        elif u < rate:
            out += [int(rng.choice(list(b"ACGT"))), base]
        else:
            out.append(base)
    at.append(len(out))
    return bytes(out), at


@functools.lru_cache(maxsize=None)
def fixture():
    rng = np.random.default_rng(20240612)
    genome = bytes(AR.random_seq(rng, SPACER + N_CHUNKS * (CHUNK_LEN + SPACER)))
    starts = [SPACER + c * (CHUNK_LEN + SPACER) for c in range(N_CHUNKS)]
    chunks = [{"id": 10 + c, "seq": genome[s:s + CHUNK_LEN].decode(), "cluster_num": 2 if c == 1 else 1, "copy_num": 2 if c < 2 else 1, "score": 0.0}
              for c, s in enumerate(starts)]
    raw_reads, encoded = [], []
    for r in range(N_READS):
        holes = set(range(starts[3] + 70, starts[3] + 130)) if r in DELETED else set()
        read, at = simulate(rng, genome, holes)
        forward = r not in REVERSE
        raw = read if forward else read.translate(COMP)[::-1]
        nodes = []
        for c, s in enumerate(starts):
            if c == 2 and r in MISSING:
                continue
            spans = [(at[s], at[s + CHUNK_LEN])]
            if c == 1 and r == DUPLICATE:
                spans.append((at[s] + 12, at[s + CHUNK_LEN] + 9))      # a second, shifted encoding of the same stretch
            for a, b in spans:
                seq = read[a:b]
                nodes.append({"position_from_start": a if forward else len(read) - b, "chunk": 10 + c, "cluster": 1 if c == 1 and r in SECOND else 0, "seq": seq.decode(),
                              "is_forward": forward, "cigar": DR.cigar_of(AR.align(AR.seq(chunks[c]["seq"]), AR.seq(seq.decode()))[0]), "posterior": [0.0] * chunks[c]["cluster_num"]})
        if not forward:
            nodes.reverse()
        raw_reads.append({"name": "read%d" % r, "desc": "", "id": r, "seq": raw.decode()})
        built = PR.nodes_to_encoded_read(r, nodes, raw.decode())
        encoded.append({k: built[k] for k in ("id", "original_length", "leading_gap", "trailing_gap", "edges", "nodes")})
    hmm = {k: 0.0 for k in ("mat_mat", "mat_ins", "mat_del", "ins_mat", "ins_ins", "ins_del", "del_mat", "del_ins", "del_del")}
    hmm.update(mat_emit=[0.0] * 16, ins_emit=[0.0] * 20)
    return {"input_file": "", "masked_kmers": {"k": 0, "thr": 0}, "coverage": "NotAvailable", "raw_reads": raw_reads, "hic_pairs": [],
            "selected_chunks": chunks, "encoded_reads": encoded, "hic_edges": [], "read_type": "CLR",
            "model_param": {"forward": hmm, "reverse": copy.deepcopy(hmm)},
            "error_rate": {k: 0.0 for k in ("del", "del_sd", "ins", "ins_sd", "mismatch", "mism_sd", "total", "total_sd")},
            "processed_stages": []}
