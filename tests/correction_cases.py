"""The problems of tests/test_correction_reference.py (CPU: oracle against the Python reference) and
tests/test_gpu_correction_reference.py (device against both).  Every case names the path of phmm_likelihood_correction.rs it is
built for, and `entered(res)` asserts on the reference's own counters that it went there (res = correction_reference.correct)."""
import copy

import numpy as np

import correction_reference as R
from helpers import correction_dataset

CASES = {}


def case(fn):
    CASES[fn.__name__] = fn
    return fn


def _all(ds):
    return [c["id"] for c in ds["chunks"]]


def _make(ds, entered, selection=None, min_gain=1e9, status=0):
    return dict(ds=ds, selection=_all(ds) if selection is None else selection, min_gain=min_gain, status=status, entered=entered)


@case
def sparse_unordered_ids():
    """chunk ids sparse and unordered, selected_chunks not in id order, read ids not in array order, selection reversed"""
    path = [7, 1000, 12, 40, 3, 500]
    ds = correction_dataset(101, path, 44, chunk_order=[1000, 7, 40, 500, 12, 3], read_id=lambda r: (r * 37) % 101 + 5)

    def entered(res):
        ids = _all(ds)
        rid = [r["id"] for r in ds["reads"]]
        assert ids != sorted(ids) and max(ids) > 10 * len(ids) and rid != sorted(rid) and len(set(rid)) == len(rid)
        assert len(res["copy_numbers"]) == 1001 and sum(1 for row in res["copy_numbers"] if row) == len(ids)
    return _make(ds, entered, selection=_all(ds)[::-1])


@case
def tandem_repeat():
    """a read holds the corrected chunk twice: two members from one read, each with the other copy in its arm"""
    ds = correction_dataset(102, [1, 2, 5, 5, 3, 4], 40, window=(4, 6))

    def entered(res):
        assert res["stats"]["members_sharing_a_read"][5] >= 5
    return _make(ds, entered)


def _strand_case(seed, strands):
    extra = [(h, strands != "reverse", [2]) for h in (0, 1, 0)]  # reads of one node: both arms empty
    ds = correction_dataset(seed, [1, 2, 3, 4], 36, window=(1, 4), strands=strands, extra_reads=extra)

    def entered(res):
        fwd, rev = res["stats"]["strands"][2]
        assert {"forward": fwd > 0 and rev == 0, "reverse": rev > 0 and fwd == 0, "mixed": fwd > 2 and rev > 2}[strands]
        assert res["stats"]["arm_pair_both_empty"] > 0          # two one-node reads against each other
        assert res["stats"]["arm_pair_with_an_empty_arm"] > res["stats"]["arm_pair_both_empty"]  # first / last in its read
    return _make(ds, entered)


@case
def one_node_reads_forward():
    """reads of one node, nodes first / last in their read; every member of the chunk forward"""
    return _strand_case(103, "forward")


@case
def one_node_reads_reverse():
    """the same, every member reverse (arms swapped on all of them)"""
    return _strand_case(104, "reverse")


@case
def one_node_reads_mixed():
    """the same, both strands on one chunk"""
    return _strand_case(105, "mixed")


@case
def unequal_and_disjoint_arms():
    """arms of 1 against 14 nodes in one job (the long one as arm1 and as arm2), and arms with no chunk in common: reads that
    leave the corrected chunk 10 into a branch (chunks 30, 31) the others do not visit"""
    path = list(range(10, 25))
    extra = [(h, f, path) for h in (0, 1) for f in (True, False)] * 2
    extra += [(h, True, [10, 11]) for h in (0, 1, 0, 1)] + [(h, f, [10, 30, 31]) for h in (0, 1) for f in (True, False)]
    ds = correction_dataset(126, path + [30, 31], 30, window=(2, 5), extra_reads=extra, chunk_order=path + [30, 31])
    for r in ds["reads"]:  # the long reads carry hard posteriors: against each other they saturate instead of crowding 1 - 1e-14
        if len(r["nodes"]) == len(path):
            for n in r["nodes"]:
                n["posterior"] = [0.0 if q == n["cluster"] else -10000.0 for q in range(2)]

    def entered(res):
        assert res["stats"]["longest_arm1_vs_arm2"][0] >= 12 and res["stats"]["longest_arm2_vs_arm1"][0] >= 12
        assert res["stats"]["arm_pair_without_common_chunk"] > 0
        assert res["per_chunk"][10]["n"] >= 14
    return _make(ds, entered, selection=[10, 11, 12])


@case
def arms_matching_after_gaps():
    """arms that match only after a gap of 1, 2 and 3 nodes: reads that lack the 1, 2 or 3 nodes next to the corrected chunk
    50; the nodes behind the gap carry hard posteriors (sim = 80 each), so that paying GAP_OPEN once and GAP_EXTEND for the rest
    beats every other alignment (tests/test_correction_reference.py::test_gap_scores works the scores out by hand)"""
    path = [50, 51, 52, 53, 54, 55, 56, 57, 58]
    extra = []
    for h in (0, 1):
        for f in (True, False):
            extra += [(h, f, path), (h, f, [50] + path[2:]), (h, f, [50] + path[3:]), (h, f, [50] + path[4:])]
    ds = correction_dataset(107, path, 0, hard=True, extra_reads=extra * 2, coverage=16.0)

    def entered(res):
        assert res["per_chunk"][50]["n"] == 32 and res["stats"]["upper_cut"] > 0
    return _make(ds, entered, selection=[50])


@case
def single_cluster_neighbours():
    """neighbours on single-cluster chunks whose estimated copy number is 1, 2 and 3 (the cps.len() == 1 branch of sim:
    +ln 2, 0, -ln 2): chunk 3 is on every read, chunk 2 on two thirds, chunk 1 on one third, haploid coverage = a third"""
    extra = []
    for r in range(36):
        ids = [3, 9] + ([2] if r % 3 != 0 else []) + ([1] if r % 3 == 1 else [])
        extra.append((r % 2, r % 4 < 2, ids))
    ds = correction_dataset(108, [3, 9, 2, 1], 0, k_of={1: 1, 2: 1, 3: 1}, extra_reads=extra, coverage=12.0)

    def entered(res):
        assert [res["copy_numbers"][c] for c in (1, 2, 3)] == [[1.0], [2.0], [3.0]]
        for cp in (1.0, 2.0, 3.0):
            assert res["stats"][("single_cluster", cp)] > 0
    return _make(ds, entered)


def _with_stray(seed, where):
    ds = correction_dataset(seed, [4, 5, 6, 8], 30, window=(2, 4))
    node = lambda cid: dict(chunk=cid, cluster=0, is_forward=True, posterior=[-0.1, -2.4])
    on5 = [r for r in ds["reads"] if r["nodes"][0]["is_forward"] and any(n["chunk"] == 5 for n in r["nodes"][:-1])]
    if where == "alone":       # ids below the largest id, each in one read only: they index empty vectors and never reach sim
        on5[0]["nodes"].append(dict(node(7), is_forward=on5[0]["nodes"][0]["is_forward"]))
        on5[1]["nodes"].insert(0, dict(node(2), is_forward=on5[1]["nodes"][0]["is_forward"]))
    elif where == "meets":     # the same id in two reads of one job: sim asserts on the lengths
        for r in on5[:2]:
            r["nodes"].append(dict(node(7), is_forward=r["nodes"][0]["is_forward"]))
    else:                      # above the largest id: obs_counts[chunk] is out of bounds
        on5[0]["nodes"].append(dict(node(9), is_forward=on5[0]["nodes"][0]["is_forward"]))
    return ds


@case
def stray_chunk_alone():
    """neighbours on chunks that are in the reads but not in `chunks`, below the largest id, never meeting their like: no effect"""
    ds = _with_stray(109, "alone")
    clean = R.correct(correction_dataset(109, [4, 5, 6, 8], 30, window=(2, 4)), [4, 5, 6, 8], 1e9)

    def entered(res):
        known = {c["id"] for c in ds["chunks"]}
        stray = [n["chunk"] for r in ds["reads"] for n in r["nodes"] if n["chunk"] not in known]
        assert sorted(stray) == [2, 7] and res["status"] == 0
        assert res["copy_numbers"][2] == [] and res["copy_numbers"][7] == []
        assert res["cluster_num"] == clean["cluster_num"]  # only MISM columns were added to two arms
    return _make(ds, entered)


@case
def stray_chunk_meets_itself():
    """the stray id meets the same id in another read of the job: sim asserts xs.len() == cps.len() (status -6)"""
    ds = _with_stray(109, "meets")

    def entered(res):
        assert res["status"] == -6 and "copy-number vector" in res["panic"]
    return _make(ds, entered, status=-6)


@case
def stray_chunk_above_largest_id():
    """the stray id is above the largest chunk id: obs_counts[chunk] is out of bounds (status -6)"""
    ds = _with_stray(109, "above")

    def entered(res):
        assert res["status"] == -6 and "obs_counts" in res["panic"]
    return _make(ds, entered, status=-6)


@case
def hard_posteriors():
    """hard posteriors [0, -10000] as a previous correction writes them: both saturations of logit_from_lnp, and
    x + y - ln cp at exactly 0 with cp == 1 (the second pass on this case's own output is test_two_passes)"""
    ds = correction_dataset(110, [1, 2, 3, 4, 5, 6], 44, hard=True, coverage=20.0)

    def entered(res):
        s = res["stats"]
        assert s["upper_cut"] > 0 and s["lower_cut"] > 0 and s["lnp_zero_with_cp_one"] > 0
        assert s.get("increment_loop_iterations", 0) == 0  # integer observations would tie exactly in the increment loop
    return _make(ds, entered)


def _cluster_nums(cov):
    k_of = {1: 2, 2: 3, 3: 4, 4: 2, 5: 1, 6: 3}
    copy_of = {1: 2, 2: 12, 3: 4, 4: 9, 5: 1, 6: 3}   # chunks 2 and 4: above the sum (increment loop); chunk 5: BELOW it
    ds = correction_dataset(111, [1, 2, 3, 4, 5, 6], 72, k_of=k_of, copy_of=copy_of, n_haps=12, window=(3, 6), coverage=cov)

    def entered(res):
        assert res["stats"]["increment_loop_iterations"] >= 1  # the increment loop ran
        assert res["stats"]["estimates_sum_above_copy_num"] >= 1 and res["copy_numbers"][5][0] >= 2.0
        assert {len(res["copy_numbers"][c]) for c in k_of} == {1, 2, 3, 4}
    return _make(ds, entered)


@case
def cluster_nums_coverage_6():
    """cluster_num 2, 3 and 4 with copy_num equal to, above and below the rounded sum of estimates; haploid coverage 6"""
    return _cluster_nums(6.0)


@case
def cluster_nums_coverage_9():
    """the same data at haploid coverage 9.3"""
    return _cluster_nums(9.3)


@case
def cluster_nums_coverage_14():
    """the same data at haploid coverage 14.2"""
    return _cluster_nums(14.2)


@case
def post_len_differs_on_a_centre():
    """a member whose post_len differs from its chunk's cluster_num: -6"""
    ds = correction_dataset(112, [1, 2, 3, 4], 30)
    node = next(n for r in ds["reads"] for n in r["nodes"] if n["chunk"] == 2)
    node["posterior"] = [-0.2, -2.0, -3.0]

    def entered(res):
        assert res["status"] == -6 and "sim:" in res["panic"]
    return _make(ds, entered, status=-6)


@case
def post_len_differs_on_a_neighbour():
    """the same on a node that is only ever a neighbour (its own chunk is not selected): -6"""
    ds = correction_dataset(112, [1, 2, 3, 4], 30)
    node = next(n for r in ds["reads"] for n in r["nodes"] if n["chunk"] == 2)
    node["posterior"] = [-0.2, -2.0, -3.0]

    def entered(res):
        assert res["status"] == -6 and "sim:" in res["panic"]
    return _make(ds, entered, selection=[1, 3], status=-6)


@case
def posterior_sums_above_one():
    """a posterior that sums above 1: logit_from_lnp asserts lnp <= 0 (-6)"""
    ds = correction_dataset(113, [1, 2, 3, 4], 30)
    for r in ds["reads"][:6]:
        for n in r["nodes"]:
            n["posterior"] = [0.5, 0.5]

    def entered(res):
        assert res["status"] == -6 and "lnp <= 0" in res["panic"]
    return _make(ds, entered, status=-6)


def _many_chunks():
    path = list(range(1, 25))
    # chunk 30 sits on single-haplotype reads only: its graph is one component, pick_k == 1, the clustering returns one cluster;
    # chunk 31 is flat on every read but one: one biased read, the adjusted Rand index on it is 0 / 0
    extra = [(0, r % 2 == 0, [28, 29, 30]) for r in range(14)]
    extra += [(r % 2, r % 2 == 0, [5, 31, 6]) for r in range(16)]
    ds = correction_dataset(114, path + [28, 29, 30, 31], 110, window=(3, 7), flat=0.25, noise=0.9, extra_reads=extra,
                            flat_chunks=(31,), chunk_order=path + [28, 29, 30, 31], coverage=12.0)
    for r in ds["reads"]:
        if any(n["chunk"] == 30 for n in r["nodes"]):
            for n in r["nodes"]:
                n["posterior"], n["cluster"] = [-0.05, -3.0], 0
    first = next(n for r in ds["reads"] for n in r["nodes"] if n["chunk"] == 31)
    first["posterior"], first["cluster"] = [-0.05, -3.0], 0
    return ds


@case
def suppression_quantile_and_one_cluster():
    """enough corrected chunks that the 5 % quantile index is >= 1, a chunk the clustering returns as one cluster, and an
    adjusted Rand index that is NaN on the biased reads (one biased read) and becomes 1"""
    ds = _many_chunks()

    def entered(res):
        assert res["stats"]["supress_pick"] >= 1 and len(res["per_chunk"]) >= 21
        assert res["per_chunk"][30]["k"] == 1 and res["cluster_num"][_all(ds).index(30)] == 1
        assert res["stats"]["ari_nan_on_biased"] >= 1 and res["per_chunk"][31]["ari"] == 1.0
        assert res["stats"]["supressed"] >= 2
    return _make(ds, entered)


def _protected(side):
    ds = _many_chunks()
    base = R.correct(ds, _all(ds), 1e9)
    # the chunk with the lowest adjusted Rand index is suppressed unless protected: min_gain on either side of its score
    cid = min((c for c in base["per_chunk"] if base["per_chunk"][c]["k"] > 1), key=lambda c: base["per_chunk"][c]["ari"])
    chunk = next(c for c in ds["chunks"] if c["id"] == cid)
    cov = sum(1 for r in ds["reads"] for n in r["nodes"] if n["chunk"] == cid)
    chunk["score"] = 20.0
    gain = 20.0 / (cov * 0.5) * (0.9 if side == "protect" else 1.1)

    def entered(res):
        idx = _all(ds).index(cid)
        if side == "protect":
            assert res["stats"].get("protected", 0) >= 1 and res["cluster_num"][idx] == 2
        else:
            assert res["cluster_num"][idx] == 1
    return _make(ds, entered, min_gain=gain)


@case
def min_gain_below_score():
    """min_gain such that cov * frac * gain is just below the score of the chunk with the lowest ARI: protected"""
    return _protected("protect")


@case
def min_gain_above_score():
    """... and just above it: suppressed"""
    return _protected("supress")


def _linked(seed, **kw):
    ds = correction_dataset(seed, [1, 2, 3, 4, 5], 40, **kw)

    def entered(res):
        # the two haplotypes are linked by similarities above 0.51: every eigenvalue in use is well apart from the next
        for pc in res["per_chunk"].values():
            lam = pc["eigenvalues"][:pc["pick_k"] + 1]
            assert min(b - a for a, b in zip(lam, lam[1:])) > 1e-3
        assert max(pc["pick_k"] for pc in res["per_chunk"].values()) >= 2
    return _make(ds, entered)


@case
def linked_haplotypes_a():
    """noisy posteriors: the haplotypes of a chunk stay linked, the small eigenvalues are distinct (a spectral gap: the
    eigenvectors are defined up to sign, so LAPACK and Jacobi must lead to the same partition)"""
    return _linked(202, flat=0.6, noise=0.4)


@case
def linked_haplotypes_b():
    """the same on other data"""
    return _linked(208, flat=0.5, noise=0.5)


def several_jobs_of_different_shape():
    """several jobs of different member count and different longest arm in ONE call (the device sizes its scratch rows by the
    longest arm of the batch, i.e. by another job than most of those it checks)"""
    path = list(range(40, 60))
    extra = [(h, f, path) for h in (0, 1) for f in (True, False)] + [(h, True, [40, 41]) for h in (0, 1)] * 6
    ds = correction_dataset(115, path, 130, window=(2, 4), extra_reads=extra, coverage=10.0)
    return _make(ds, lambda res: None, selection=[40, 45, 50, 59])


def more_pairs_than_threads(n_per_chunk=300, n_chunks=4):
    """one call whose ordered pairs exceed the kernel's 262,144 threads: several chunks of about 300 members each"""
    path = list(range(1, n_chunks + 3))
    ds = correction_dataset(116, path, 0, extra_reads=[(r % 2, r % 3 != 0, path[(r % 3):len(path) - (r % 2)]) for r in range(n_per_chunk)],
                            coverage=n_per_chunk / 2.0)
    return _make(ds, lambda res: None, selection=path[2:2 + n_chunks])


def two_pass_input(res, made):
    """the DataSet after the first pass (reference's write-back), for the second"""
    ds = copy.deepcopy(made["ds"])
    e = 0
    for read in ds["reads"]:
        for n in read["nodes"]:
            n["cluster"], n["posterior"] = res["cluster"][e], list(res["posterior"][e])
            e += 1
    for c, k in zip(ds["chunks"], res["cluster_num"]):
        c["cluster_num"] = k
    return ds
