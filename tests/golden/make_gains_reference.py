"""Writes tests/golden/gains_reference/: what tests/gains_reference.py computes on the cases of tests/gains_cases.py.

    python tests/golden/make_gains_reference.py [processes, default 8]

<case>.json holds the case's arguments, per simulation the digests of its sequences, of every pair's ops and of every pair's
distance, its median, null count, margin and scale, and the final numbers; <case>.<k>.npy hold the likelihoods, one per distinct
(strand, template, read) of a simulation in order of first appearance, simulation after simulation, in pieces of 18,000 doubles.
The output does not depend on the number of processes.  What a case is for is asserted here, on the reference alone, before
anything is written: reads of length 0 and 1, anti-diagonals of 65 cells and of more than 192, a distance above 127, a read
beyond 250 bases, a floor that decides and one that does
not, and that no decision of the reference (gains_reference: `margin`) sits within 100 x the likelihood bound of its threshold.

Run time: 2 minutes on 8 processes, 13.5 CPU-minutes (1,200 simulations of 200 pairs at 0.5 to 0.9 s each; the 100,004 pairs of
two_batches are 1,400 distinct ones).
"""
import multiprocessing
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import gains_cases as K  # noqa: E402
import gains_reference as G  # noqa: E402


def _facts(sim):
    lens = [len(r) for r in sim["reads"]]
    return dict(len0=lens.count(0), len1=lens.count(1), longest=max(lens + [len(t) for t in sim["tmpls"]]),
                max_dist=max(d for row in sim["dist"] for d in row), max_diagonal=max(min(len(t), n) for t in sim["tmpls"] for n in lens))


def _job(job):
    kind, name, q, i = job
    if kind == "gains":
        model, seed, seq_len, band, homop_len = K.GAINS_CASES[name]
        f, r = K.models()[model]
        ty, length = G.profiles(homop_len)[q]
        sim = G.gain_simulation(f, r, seed, seq_len, band, length, ty, i)
    else:
        sim = K.min_gain_sample(name, i)
    e, lk = K.sim_entry(sim)
    return job, e, lk, _facts(sim)


def main():
    procs = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    jobs = []
    for name, (_, _, _, _, homop_len) in K.GAINS_CASES.items():
        jobs += [("gains", name, q, i) for q in range(len(G.profiles(homop_len))) for i in range(G.SAMPLE_NUM)]
    for name, (_, _, sample_num, _, _, _) in K.MIN_GAIN_CASES.items():
        jobs += [("min_gain", name, 0, s) for s in range(sample_num)]
    jobs.sort(key=lambda j: j[1] != "two_batches")          # the longest jobs first
    with multiprocessing.Pool(procs) as pool:
        done = dict((job, rest) for job, *rest in pool.imap_unordered(_job, jobs))
    index = {}
    for name, args in list(K.GAINS_CASES.items()) + list(K.MIN_GAIN_CASES.items()):
        kind = "gains" if name in K.GAINS_CASES else "min_gain"
        mine = sorted(j for j in done if j[1] == name)                      # batch order: profile, simulation
        entries, lks, facts = zip(*(done[j] for j in mine))
        case = dict(kind=kind, args=list(args), sims=list(entries))
        for key in ("len0", "len1"):
            case[key] = sum(f[key] for f in facts)
        for key in ("longest", "max_dist", "max_diagonal"):
            case[key] = max(f[key] for f in facts)
        case["status"] = "unsupported" if case["longest"] > K.MAX_DEVICE_LEN else "ok"    # (what the device answers)
        assert (case["status"] == "unsupported") == (name == "too_long"), (name, case["longest"])
        margin, exact = min(e["margin"] for e in entries), min(e["exact_margin"] for e in entries)
        if kind == "gains":
            profiles = G.profiles(args[4])
            case["profiles"] = [list(p) for p in profiles]
            case["gain"], case["prob"] = [], []
            for q in range(len(profiles)):
                ss = entries[q * G.SAMPLE_NUM:(q + 1) * G.SAMPLE_NUM]
                gain, prob = G.profile_of([e["median"] for e in ss], [e["null"] for e in ss])
                case["gain"].append(gain)
                case["prob"].append(prob)
                margin = min(margin, G._gap([e["median"] for e in ss], G.GAIN_POS))
        else:
            case["batches"] = G.batch_sizes(args[2], args[3])
            case["min_gain"], m, floor = G.minimum_gain_of([e["median"] for e in entries])
            case["floor_decides"] = sorted(e["median"] for e in entries)[2] < G.MIN_REQ
            margin, exact = min(margin, m), min(exact, floor)
        case["margin"], case["exact_margin"], case["scale"] = margin, exact, max(e["scale"] for e in entries)
        assert exact >= margin >= K.MARGIN_FACTOR * K.bound_of(case["scale"]), (name, margin, exact, case["scale"])
        flat = np.array([v for lk in lks for v in lk], dtype="<f8")
        assert len(flat) == sum(e["distinct"] for e in entries) and np.all(np.isfinite(flat)), name
        case["pieces"] = (len(flat) + K.PIECE - 1) // K.PIECE
        os.makedirs(K.GOLDEN_DIR, exist_ok=True)
        for k in range(case["pieces"]):
            np.save(os.path.join(K.GOLDEN_DIR, "%s.%d.npy" % (name, k)), flat[k * K.PIECE:(k + 1) * K.PIECE])
        index[name] = case
    # what the cases are for
    assert index["len6_deletions"]["len0"] > 0 and index["len6_deletions"]["len1"] > 0, index["len6_deletions"]
    assert index["top_bit"]["max_dist"] > 127, index["top_bit"]["max_dist"]
    assert index["two_batches"]["batches"] == [3, 1]
    assert index["second_stride"]["max_diagonal"] >= 65 and index["upper_bound"]["max_diagonal"] > 192
    floors = [c["floor_decides"] for c in index.values() if "floor_decides" in c]
    assert True in floors and False in floors, floors
    for name, case in index.items():
        K.dump_case(name, case)
    for name, c in index.items():
        print(name, c["status"], "sims", len(c["sims"]), "pieces", c.get("pieces"), "margin", c.get("margin"), "exact_margin", c.get("exact_margin"), "scale", c.get("scale"),
              "len0", c["len0"], "len1", c["len1"], "longest", c["longest"], "max_dist", c["max_dist"],
              "floor", c.get("floor_decides"), "result", c.get("gain"), c.get("prob"), c.get("min_gain"))


if __name__ == "__main__":
    main()
