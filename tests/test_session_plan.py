"""jtk_amd/csrc/session_plan.h compiled as plain C++ (no HIP, no GPU) with AddressSanitizer and UBSan: the host-only plan of a
resident batch -- every ReadMeta / ChunkMeta / ChunkState field, the buffer totals, the pair-kernel item list, the wide-band
census, the chain's three launch classes with their evictions and workspace offsets, the wave and stripe counts and the
refusals -- against a restatement written here from the rules (the strides of device_common.h's kernels, the coverage rule of
mod.rs:108-111, radius = ceil(len * band_frac) / 2, classes by mcmc_lds_bytes as test_chain_layout.py restates it).  Everything
the program prints is compared exactly.  Every case named for an arm asserts, from the restatement, that it takes that arm."""
import math
import os
import subprocess

import pytest

from test_chain_layout import expected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "jtk_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")

INVALID_ARG, UNSUPPORTED = -1, -3
NUM_ROW, ACC_N, MAX_COPY, MAX_DIM, MAX_PILEUP = 14, 16, 7, 21, 1023
PAIR_MAX_RADIUS, MAX_RADIUS, WIDE_MAX_RADIUS, SCRATCH_GUARD = 14, 30, 255, 16
KIB80, KIB160 = 80 * 1024, 160 * 1024

PROGRAM = r'''
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <iostream>
#include "session_plan.h"

static double hexd() { std::string t; std::cin >> t; return strtod(t.c_str(), nullptr); }
template <class T> static void row(const char *tag, const std::vector<T> &v) {
    printf("%s", tag);
    for (auto x : v) printf(" %" PRIu64, (uint64_t)x);
    printf("\n");
}
static void batch_case(const std::string &name) {
    jtk_lc_params_t params;
    memset(&params, 0, sizeof params);
    params.band_frac = hexd();
    params.haploid_coverage = hexd();
    uint32_t H, post_stride; int polish_only, has_extra; size_t n_chunks;
    std::cin >> H >> post_stride >> polish_only >> has_extra >> n_chunks;
    params.gains.max_homopolymer_len = H;
    std::vector<jtk_lc_chunk_t> chunks(n_chunks);
    std::vector<ChunkExtra> extra(n_chunks);
    uint64_t n_reads = 0;
    for (size_t c = 0; c < n_chunks; c++) {
        memset(&chunks[c], 0, sizeof chunks[c]);
        memset(&extra[c], 0, sizeof extra[c]);
        std::cin >> chunks[c].chunk_id >> chunks[c].copy_num >> chunks[c].n_reads >> chunks[c].tmpl_len >> chunks[c].read_first;
        chunks[c].tmpl_off = 1000 * c;
        if (has_extra) {
            std::cin >> extra[c].radius;
            extra[c].local_coverage = hexd();
            std::cin >> extra[c].take_num;
        }
        n_reads += chunks[c].n_reads;
    }
    // the offsets do not start at 0: only their differences may matter
    std::vector<uint64_t> read_off(n_reads + 1, 5), ops_off(n_reads + 1, 11);
    std::vector<uint8_t> strand(n_reads);
    for (uint64_t g = 0; g < n_reads; g++) {
        uint64_t rl, ol; unsigned st;
        std::cin >> rl >> ol >> st;
        read_off[g + 1] = read_off[g] + rl;
        ops_off[g + 1] = ops_off[g] + ol;
        strand[g] = (uint8_t)st;
    }
    BatchPlan bp;
    std::string msg;
    const int rc = plan_batch(params, n_chunks, chunks.data(), read_off.data(), ops_off.data(), strand.data(), post_stride,
                              has_extra ? extra.data() : nullptr, polish_only != 0, bp, msg);
    printf("CASE %s\nRC %d |%s\n", name.c_str(), rc, msg.c_str());
    size_t n_cfg;
    std::cin >> n_cfg;
    std::vector<std::pair<uint32_t, SweepSizes>> cfg(n_cfg);
    for (auto &w : cfg) std::cin >> w.first >> w.second.phmm_lds_bytes >> w.second.phmm_pair_lds_bytes >> w.second.phmm_wide_lds_bytes >> w.second.phmm_wide_scratch_doubles;
    if (rc) return;
    for (size_t c = 0; c < bp.chunks.size(); c++) {
        const ChunkMeta &m = bp.chunks[c];
        printf("C %" PRIu64 " %u %u %u %u %" PRIu64 " %" PRIu64 " %u %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %a %u %u\n", m.chunk_id, m.copy_num,
               m.n_reads, m.read_first, m.tmpl_cap, m.tmpl_off, m.total_off, m.radius, m.edit_cap, m.edit_off, m.feat_off, m.cand_off,
               m.local_coverage, m.take_num, m.pad0);
        const ChunkState &s = bp.state0[c];
        printf("S %u %u %u %u %d %u %u %u %a %" PRIu64 " %" PRIu64 " %u %u\n", s.tmpl_len, s.buf, s.active, s.rounds, s.status, s.n_edits,
               s.dim, s.k, s.score, s.draws, s.chain_cycles, s.chain_events, s.chain_pad);
    }
    for (const ReadMeta &r : bp.reads)
        printf("R %u %u %" PRIu64 " %" PRIu64 " %u %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", r.chunk, r.read_len, r.ey_off, r.ops_off,
               r.ops_cap, r.strand, r.delta_off, r.table_off, r.raw_off, r.row_off);
    row("COPY0", bp.copy0);
    row("OPSLEN", bp.opslen);
    row("HOMOP", bp.homop_off);
    row("AUX", bp.aux_off);
    row("LG", bp.lg_off);
    row("TOTALS", std::vector<uint64_t>{bp.n_reads, bp.tmpl, bp.ops, bp.ey, bp.delta, bp.raw, bp.row, bp.total, bp.edit, bp.feat, bp.cand, bp.aux, bp.lg});
    row("MAXIMA", std::vector<uint64_t>{bp.max_tmpl, bp.max_read, bp.max_n, bp.max_copy, bp.n_wide_reads, bp.max_wide_radius, bp.has_split});
    row("PAIRS", bp.pair_items);
    row("ORDER", bp.chain.order);
    for (const ChainClass &k : bp.chain.cls) row("CLASS", std::vector<uint64_t>{k.first, k.count, k.lds_n, k.lds_d, k.lds_k, k.lds_bytes});
    row("WSOFF", bp.chain.ws_off);
    row("WSBYTES", std::vector<uint64_t>{bp.chain.ws_bytes});
    for (auto &w : cfg) {
        WavePlan wp;
        msg.clear();
        const int wrc = plan_waves(w.first, w.second, bp, wp, msg);
        if (wrc) printf("WAVES %d |%s\n", wrc, msg.c_str());
        else printf("WAVES 0 %u %" PRIu64 " %u %u %u %" PRIu64 " |\n", wp.n_waves, wp.stripe_stride, wp.n_stripes, wp.n_pair_waves, wp.n_wide_waves, wp.wide_stride);
    }
}
static void feature_case(const std::string &name) {
    uint32_t max_k; size_t limit, n_chunks;
    std::cin >> max_k >> limit >> n_chunks;
    std::vector<jtk_lc_feature_chunk_t> chunks(n_chunks);
    std::vector<uint8_t> failed(n_chunks);
    for (size_t c = 0; c < n_chunks; c++) {
        unsigned f;
        memset(&chunks[c], 0, sizeof chunks[c]);
        std::cin >> chunks[c].copy_num >> chunks[c].n_reads >> chunks[c].dim >> f;
        failed[c] = (uint8_t)f;
    }
    FeatureChainPlan fp;
    plan_feature_chain(n_chunks, chunks.data(), failed, max_k, limit, fp);
    printf("CASE %s\n", name.c_str());
    row("ORDER", fp.order);
    row("LAUNCH", std::vector<uint64_t>{fp.n_lds, fp.n_ws, fp.lds.n, fp.lds.d, fp.lds.k, fp.ws.n, fp.ws.d, fp.ws.k});
    row("WSOFF", fp.ws_off);
    row("WSBYTES", std::vector<uint64_t>{fp.ws_bytes});
}
int main() {
    std::string kind, name;
    while (std::cin >> kind >> name) {
        if (kind == "B") batch_case(name);
        else if (kind == "F") feature_case(name);
        else return 2;
    }
    // the chunk's dimensions as the trace entry point asks for them
    for (uint32_t copy = 0; copy <= 9; copy++) {
        ChunkMeta cm;
        memset(&cm, 0, sizeof cm);
        cm.copy_num = copy;
        cm.n_reads = 10 + copy;
        const ChainDims x = chain_dims_of(cm);
        printf("DIMS %u %u %u %u\n", copy, x.n, x.d, x.k);
    }
    // which variant filter a pass takes
    for (int polish_only = 0; polish_only < 2; polish_only++)
        for (uint32_t n : {0u, 1u, 65535u, 65536u, 0xffffffffu})
            printf("TABLES %d %u %d\n", polish_only, n, (int)batch_needs_tables(polish_only != 0, n));
    return 0;
}
'''


# ---- the cases

def chunk(copy, n, tl, chunk_id=None, read_first=None, extra=None):
    return dict(copy=copy, n=n, tl=tl, chunk_id=chunk_id, read_first=read_first, extra=extra)


DEFAULT_WAVES = [(256, 14336, 20480, 61440, 500000), (2, 14336, 20480, 61440, 500000), (256, 14336, 90000, 50000, 1 << 30)]


def case(name, chunks, band_frac=0.125, hap=20.0, H=4, post_stride=8, polish_only=False, waves=None):
    """Fills in ids, read_first and the reads: lengths that differ read by read and are no multiple of anything."""
    first, reads = 0, []
    for i, ch in enumerate(chunks):
        if ch["chunk_id"] is None:
            ch["chunk_id"] = 1000 + 7 * i
        if ch["read_first"] is None:
            ch["read_first"] = first
        first += ch["n"]
        for r in range(ch["n"]):
            g = len(reads)
            rl = max(1, ch["tl"] + (g * 7) % 11 - 5)
            reads.append((rl, rl + (g * 3) % 13, (g // 2 + g) & 1))
    extras = [ch["extra"] is not None for ch in chunks]
    assert all(extras) or not any(extras)
    return dict(name=name, chunks=chunks, band_frac=band_frac, hap=hap, H=H, post_stride=post_stride, polish_only=polish_only,
                has_extra=bool(chunks) and all(extras), reads=reads, waves=DEFAULT_WAVES if waves is None else waves)


def batch_cases():
    X = lambda radius, cov, take: dict(radius=radius, cov=cov, take=take)  # noqa: E731
    return [
        case("empty", []),
        case("no_reads_between", [chunk(2, 3, 300), chunk(2, 0, 211), chunk(3, 2, 333)]),
        case("copies_2_7_8", [chunk(2, 9, 300), chunk(7, 30, 310), chunk(8, 40, 320)], hap=4.5),
        case("extra", [chunk(2, 5, 300, extra=X(14, 2.5, 0)), chunk(4, 4, 290, extra=X(14, 7.25, 0)), chunk(8, 6, 310, extra=X(14, 1.0, 3)),
                       chunk(3, 4, 300, extra=X(15, 3.0, 0)), chunk(2, 3, 280, extra=X(14, 0.5, 7)), chunk(2, 7, 280, extra=X(40, 0.5, 2))],
             post_stride=4),
        case("radii_14_15", [chunk(2, 5, 224), chunk(2, 4, 232), chunk(2, 6, 240), chunk(2, 1, 225)]),
        case("radii_30_31", [chunk(2, 5, 480), chunk(2, 9, 496), chunk(2, 4, 300)]),
        case("radii_255_256", [chunk(2, 3, 4080), chunk(2, 2, 4096), chunk(2, 3, 200)]),
        case("pileups_1023_1024", [chunk(2, 1024, 100), chunk(2, 1023, 90), chunk(3, 1024, 80), chunk(2, 20, 100)]),
        case("evict_at_80k", [chunk(2, 30, 120), chunk(2, 500, 100), chunk(7, 100, 110)]),
        case("evict_at_160k", [chunk(7, 300, 100), chunk(2, 1000, 90), chunk(2, 30, 120)]),
        case("polish_only", [chunk(2, 1024, 100), chunk(7, 100, 110), chunk(2, 5, 224)], polish_only=True),
        case("err_not_contiguous", [chunk(2, 3, 300), chunk(2, 2, 300, read_first=4)]),
        case("err_post_stride", [chunk(2, 3, 300), chunk(5, 2, 300)], post_stride=4),
        case("err_post_stride_sub_problem", [chunk(8, 3, 300, extra=X(20, 1.0, 0)), chunk(5, 2, 300, extra=X(20, 1.0, 0))], post_stride=4),
        case("post_stride_spares_empty_chunks", [chunk(2, 3, 300), chunk(5, 0, 300)], post_stride=4),
        case("refusals", [chunk(2, 5, 224), chunk(2, 9, 496)],
             waves=[(256, 14336, KIB160 + 1, 61440, 500000), (256, 14336, KIB160, KIB160 + 1, 500000), (256, KIB160 + 1, KIB160, KIB160, 500000),
                    (256, KIB160 + 1, KIB160 + 1, KIB160 + 1, 500000), (256, KIB160 + 1, 20480, KIB160 + 1, 500000), (256, KIB160, KIB160, KIB160, 500000)]),
    ]


FEATURE_CASES = [
    # (name, max_k, [(copy, n_reads, dim, failed)]): deep x narrow, shallow x wide and a bystander fit one by one, not together
    ("features_evict", 7, [(2, 1000, 2, 0), (9, 50, 3, 1), (7, 300, 21, 0), (2, 10, 2, 0), (2, 1024, 1, 0), (2, 5, 30, 1), (2, 1023, 10, 0)]),
    ("features_empty", 2, []),
    ("features_all_fit", 4, [(4, 60, 12, 0), (2, 0, 0, 0), (3, 40, 9, 0)]),
]


def stdin_of(cases):
    out = []
    for cs in cases:
        out.append("B %s %s %s %d %d %d %d %d" % (cs["name"], float(cs["band_frac"]).hex(), float(cs["hap"]).hex(), cs["H"], cs["post_stride"],
                                                  cs["polish_only"], cs["has_extra"], len(cs["chunks"])))
        for ch in cs["chunks"]:
            row = "%d %d %d %d %d" % (ch["chunk_id"], ch["copy"], ch["n"], ch["tl"], ch["read_first"])
            if cs["has_extra"]:
                row += " %d %s %d" % (ch["extra"]["radius"], float(ch["extra"]["cov"]).hex(), ch["extra"]["take"])
            out.append(row)
        out.extend("%d %d %d" % r for r in cs["reads"])
        out.append(str(len(cs["waves"])))
        out.extend("%d %d %d %d %d" % w for w in cs["waves"])
    for name, max_k, chunks in FEATURE_CASES:
        out.append("F %s %d %d %d" % (name, max_k, KIB160, len(chunks)))
        out.extend("%d %d %d %d" % c for c in chunks)
    return "\n".join(out) + "\n"


# ---- the restatement

def lds_bytes(n, d, k):
    return expected(n, d, k)[1]


def ws_bytes(n, d, k):
    return expected(n, d, k)[2]


def chain_dims(copy, n):
    """one clustering() call: max(copy, 2) clusters at most (7 at most), three picked columns per cluster"""
    return n, min(MAX_DIM, 3 * max(copy, 2)), min(max(copy, 2), MAX_COPY)


def maxima(members, dims, floor=(0, 0, 0)):
    return tuple(max([floor[i]] + [dims[c][i] for c in members]) for i in range(3))


def fit(members, dims, limit, worst_key, floor=(0, 0, 0)):
    """a launch is sized for its members' maxima; while those exceed the limit, the first of the worst members leaves"""
    members, gone = list(members), []
    while members and lds_bytes(*maxima(members, dims, floor)) > limit:
        w = max(members, key=worst_key)
        members.remove(w)
        gone.append(w)
    return members, gone


def restate_chain(metas):
    """metas: (copy_num of one clustering() call, n_reads) per chunk -> order, three class records, workspace offsets, evictions"""
    dims = [chain_dims(c, n) for c, n in metas]
    need = [lds_bytes(*x) for x in dims]
    cls = [[], [], []]
    for c, (_, n) in enumerate(metas):
        cls[2 if n > MAX_PILEUP else (0 if need[c] <= KIB80 else 1)].append(c)
    order, records, evictions = [], [], []
    for q, limit in ((0, KIB80), (1, KIB160)):
        stay, gone = fit(cls[q], dims, limit, lambda c: need[c])
        cls[q + 1] += gone
        evictions.append(gone)
        m = maxima(stay, dims)
        stay = sorted(stay, key=lambda c: -(metas[c][1] * min(metas[c][0], 4)))  # longest chains first; stable
        records.append((len(order), len(stay)) + m + (lds_bytes(*m) if stay else 0,))
        order += stay
    records.append((len(order), len(cls[2])) + maxima(cls[2], dims) + (0,))
    order += cls[2]
    ws_off, ws = [], 0
    for c in cls[2]:
        ws_off.append(ws)
        ws += ws_bytes(*dims[c])
    return order, records, ws_off, ws, evictions


def restate_batch(cs):
    chunks, reads = cs["chunks"], cs["reads"]
    running = 0
    for ch in chunks:
        if ch["read_first"] != running:
            return dict(rc=INVALID_ARG, msg="chunks must list their reads contiguously in order")
        rows = (4 if ch["copy"] > MAX_COPY else ch["copy"]) if cs["has_extra"] else ch["copy"]   # a sub-problem is one clustering() call
        if rows > cs["post_stride"] and ch["n"] > 0:
            return dict(rc=INVALID_ARG, msg="post_stride smaller than a chunk's copy_num")
        running += ch["n"]
    out = dict(rc=0, msg="", C=[], S=[], R=[], COPY0=[], OPSLEN=[], HOMOP=[], AUX=[], LG=[], PAIRS=[])
    tmpl = ops = ey = delta = raw = rowo = total = edit = feat = cand = aux = lg = 0
    max_tmpl = max_read = max_n = max_copy = n_wide = max_wide = 0
    g = 0
    for i, ch in enumerate(chunks):
        tl, n, copy = ch["tl"], ch["n"], ch["copy"]
        cap = tl + tl // 8 + 64
        one_call = 4 if copy > MAX_COPY else copy
        per_cluster = n / copy
        cov = per_cluster if copy <= 2 else max(per_cluster, cs["hap"])
        radius, take = math.ceil(tl * cs["band_frac"]) // 2, 0
        if cs["has_extra"]:
            radius, cov, take = ch["extra"]["radius"], ch["extra"]["cov"], ch["extra"]["take"]
        status = UNSUPPORTED if radius > WIDE_MAX_RADIUS else 0
        if MAX_RADIUS < radius <= WIDE_MAX_RADIUS:
            n_wide += n
            max_wide = max(max_wide, radius)
        out["C"].append((ch["chunk_id"], one_call, n, g, cap, tmpl, total, radius, cap // 2 + 2, edit, feat, cand, cov, take, 0))
        out["S"].append((tl, 0, 1, 0, status, 0, 0, 1, 0.0, 0, 0, 0, 0))
        out["COPY0"].append(copy)
        out["HOMOP"].append(tmpl)
        out["AUX"].append(aux)
        out["LG"].append(lg)
        if radius <= PAIR_MAX_RADIUS and status == 0:
            voters = min(take, n) if take else n
            out["PAIRS"] += [g + r for r in range(0, voters - 1, 2)]
            if voters % 2:
                out["PAIRS"].append((g + voters - 1) | 0x80000000)
        for _ in range(n):
            rl, ol, st = reads[g]
            slot = (ol + tl // 8 + 64 + 7) & ~7
            out["R"].append((i, rl, ey, ops, slot, 1 if st else 0, delta, raw, raw, rowo))
            out["OPSLEN"].append(ol)
            max_read = max(max_read, rl)
            ey += rl + 1
            ops += slot
            delta += ((cap + rl) >> 6) + 3
            raw += ACC_N * (cap + 1)
            rowo += cap + 1
            g += 1
        max_tmpl, max_n, max_copy = max(max_tmpl, cap), max(max_n, n), max(max_copy, one_call)
        tmpl += cap
        total += NUM_ROW * (cap + 1)
        cand += NUM_ROW * (cap + 1)
        edit += cap // 2 + 2
        feat += n * MAX_DIM
        aux += 3 * cs["H"] * (n + 1) + (n + 1) + (MAX_COPY + 2)
        lg += n * (MAX_COPY + 1)
    out["TOTALS"] = [g, tmpl, ops, ey, delta, raw, rowo, total, edit, feat, cand, aux, lg]
    out["MAXIMA"] = [max_tmpl, max_read, max_n, max_copy, n_wide, max_wide, int(any(ch["copy"] > MAX_COPY for ch in chunks))]
    if cs["polish_only"]:
        order, records, ws_off, ws, evictions = [], [(0, 0, 0, 0, 0, 0)] * 3, [], 0, [[], []]
    else:
        order, records, ws_off, ws, evictions = restate_chain([(c[1], c[2]) for c in out["C"]])
    out["ORDER"], out["CLASS"], out["WSOFF"], out["WSBYTES"], out["evictions"] = order or [0], records, ws_off, [ws], evictions
    out["WAVES"] = [restate_waves(w, out) for w in cs["waves"]]
    return out


def restate_waves(cfg, plan):
    n_cu, phmm, pair, wide, scratch = cfg
    n_reads, max_tmpl, max_read, n_wide = plan["TOTALS"][0], plan["MAXIMA"][0], plan["MAXIMA"][1], plan["MAXIMA"][4]
    n_waves = max(1, min(n_reads, n_cu * min(max(KIB160 // phmm, 1), 12)))
    n_pair = n_wide_waves = wide_stride = 0
    if plan["PAIRS"]:
        if pair > KIB160:
            return (UNSUPPORTED, "template + reads too long for the LDS staging of phmm_pair_kernel")
        n_pair = min(len(plan["PAIRS"]), n_cu * min(KIB160 // pair, 8), n_waves)
    if n_wide:
        if wide > KIB160:
            return (UNSUPPORTED, "template + read too long for the LDS staging of phmm_wide_kernel")
        want, budget = n_cu * min(KIB160 // wide, 4), (48 << 30) // (scratch * 8)
        if want > budget:
            want = budget or 1
        n_wide_waves, wide_stride = min(n_wide, want), scratch
    if phmm > KIB160:
        return (UNSUPPORTED, "template + read too long for the LDS staging of phmm_kernel")
    return (0, n_waves, (max_tmpl + max_read + 8 + SCRATCH_GUARD) * 128, n_cu * 16, n_pair, n_wide_waves, wide_stride, "")


def restate_features(max_k, chunks):
    dims = [(max(1, n), max(1, d), max(2, copy)) for copy, n, d, _ in chunks]
    ok = [c for c, ch in enumerate(chunks) if not ch[3]]
    in_ws = [c for c in ok if chunks[c][1] > MAX_PILEUP or lds_bytes(*dims[c]) > KIB160]
    in_lds, gone = fit([c for c in ok if c not in in_ws], dims, KIB160, lambda c: chunks[c][1] * max(1, chunks[c][2]), floor=(1, 1, max_k))
    in_ws = sorted(in_ws + gone)
    failed = [c for c, ch in enumerate(chunks) if ch[3]]
    ws_off, ws = [], 0
    for c in in_ws:
        ws_off.append(ws)
        ws += ws_bytes(*dims[c])
    # (the failed chunks are spliced in one by one at the same place: the last one comes first)
    return dict(ORDER=in_lds + failed[::-1] + in_ws, WSOFF=ws_off, WSBYTES=[ws], evicted=gone,
                LAUNCH=[len(in_lds) + len(failed), len(in_ws)] + list(maxima(in_lds, dims, (1, 1, max_k))) + list(maxima(in_ws, dims, (1, 1, max_k))))


# ---- the program, once

@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("session_plan")
    src, exe = tmp / "plan.cpp", tmp / "plan"
    src.write_text(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-I", CSRC,
                           "-I", INCLUDE, str(src), "-o", str(exe)])
    cases = batch_cases()
    run = subprocess.run([str(exe)], input=stdin_of(cases).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert run.returncode == 0, run.stderr.decode()[-4000:]
    assert run.stderr == b"", run.stderr.decode()[-4000:]   # (a sanitizer report that did not end the run)
    got, cur = {}, None
    for line in run.stdout.decode().splitlines():
        tag, _, rest = line.partition(" ")
        if tag == "CASE":
            cur = got.setdefault(rest, {})
        elif tag in ("DIMS", "TABLES"):
            got.setdefault(tag, []).append(tuple(map(int, rest.split())))
        else:
            cur.setdefault(tag, []).append(rest)
    return {cs["name"]: cs for cs in cases}, got


def parse_batch(raw):
    rc, _, msg = raw["RC"][0].partition(" |")
    if int(rc):
        assert set(raw) == {"RC"}
        return dict(rc=int(rc), msg=msg)
    ints = lambda s: [int(x) for x in s.split()]  # noqa: E731
    out = dict(rc=0, msg=msg)
    for tag, at in (("C", 12), ("S", 8)):   # one float each, printed exactly (%a)
        out[tag] = [tuple(float.fromhex(x) if j == at else int(x) for j, x in enumerate(r.split())) for r in raw.get(tag, [])]
    out["R"] = [tuple(ints(r)) for r in raw.get("R", [])]
    for tag in ("COPY0", "OPSLEN", "HOMOP", "AUX", "LG", "TOTALS", "MAXIMA", "PAIRS", "ORDER", "WSOFF", "WSBYTES"):
        (row,) = raw[tag]
        out[tag] = ints(row)
    out["CLASS"] = [tuple(ints(r)) for r in raw["CLASS"]]
    out["WAVES"] = []
    for r in raw["WAVES"]:
        nums, _, msg = r.partition(" |")
        out["WAVES"].append(tuple(ints(nums)) + (msg,))
    return out


BATCH_NAMES = [cs["name"] for cs in batch_cases()]


@pytest.mark.parametrize("name", BATCH_NAMES)
def test_plan_matches_the_restatement(program_output, name):
    cases, got = program_output
    want = restate_batch(cases[name])
    have = parse_batch(got[name])
    evictions = want.pop("evictions", None)
    assert sorted(have) == sorted(want)
    for key in sorted(want):
        assert have[key] == want[key], (name, key)
    # ---- the case takes the arm it is named for: asked of the restatement
    radii = [c[7] for c in want.get("C", [])]
    if name == "empty":
        assert want["TOTALS"] == [0] * 13 and want["ORDER"] == [0] and want["WAVES"][0][1] == 1
    elif name == "no_reads_between":
        assert [c[2] for c in want["C"]] == [3, 0, 2] and want["C"][2][3] == 3
    elif name == "copies_2_7_8":
        assert want["COPY0"] == [2, 7, 8] and [c[1] for c in want["C"]] == [2, 7, 4] and want["MAXIMA"][6] == 1 and want["MAXIMA"][3] == 7
        assert [c[12] for c in want["C"]] == [4.5, 4.5, 5.0] and 30 / 7 < 4.5   # diploid: reads per copy; raised to haploid_coverage; above it
    elif name == "extra":
        assert radii == [14, 14, 14, 15, 14, 40] and [c[12] for c in want["C"]] == [2.5, 7.25, 1.0, 3.0, 0.5, 0.5] and [c[13] for c in want["C"]] == [0, 0, 3, 0, 7, 2]
        # odd, even, cut to 3 by take_num, radius 15 left out, take_num beyond the read count, a wide chunk
        assert want["PAIRS"] == [0, 2, 4 | 1 << 31, 5, 7, 9, 11 | 1 << 31, 19, 21 | 1 << 31]
    elif name == "radii_14_15":
        assert radii == [14, 14, 15, 14] and want["PAIRS"] == [0, 2, 4 | 1 << 31, 5, 7, 15 | 1 << 31] and want["MAXIMA"][4] == 0
    elif name == "radii_30_31":
        assert radii == [30, 31, 19] and want["MAXIMA"][4:6] == [9, 31] and want["PAIRS"] == []
        assert [w[5] for w in want["WAVES"]] == [9, 4, 6]      # every wide read; 2 CUs x 2 waves; the 48 GB budget
    elif name == "radii_255_256":
        assert radii == [255, 256, 12] and [s[4] for s in want["S"]] == [0, UNSUPPORTED, 0] and want["MAXIMA"][4:6] == [3, 255]
        assert want["PAIRS"] == [5, 7 | 1 << 31]
    elif name == "pileups_1023_1024":
        assert want["ORDER"] == [3, 1, 0, 2] and [k[:2] for k in want["CLASS"]] == [(0, 1), (1, 1), (2, 2)] and evictions == [[], []]
        assert want["WSOFF"] == [0, ws_bytes(1024, 6, 2)] and want["WSBYTES"] == [ws_bytes(1024, 6, 2) + ws_bytes(1024, 9, 3)]
    elif name == "evict_at_80k":
        # each of the two fits 80 KiB, their maxima do not: the larger by its own need (the deep diploid one) moves to class 1
        assert lds_bytes(500, 6, 2) <= KIB80 and lds_bytes(100, 21, 7) <= KIB80 < lds_bytes(500, 21, 7) and lds_bytes(500, 6, 2) > lds_bytes(100, 21, 7)
        assert evictions == [[1], []] and want["ORDER"] == [2, 0, 1] and [k[:2] for k in want["CLASS"]] == [(0, 2), (2, 1), (3, 0)]
        assert want["CLASS"][0][2:5] == (100, 21, 7) and want["CLASS"][1][2:5] == (500, 6, 2)
    elif name == "evict_at_160k":
        assert KIB80 < lds_bytes(300, 21, 7) < lds_bytes(1000, 6, 2) <= KIB160 < lds_bytes(1000, 21, 7)
        assert evictions == [[], [1]] and want["ORDER"] == [2, 0, 1] and [k[:2] for k in want["CLASS"]] == [(0, 1), (1, 1), (2, 1)]
        assert want["CLASS"][2][2:] == (1000, 6, 2, 0) and want["WSOFF"] == [0] and want["WSBYTES"] == [ws_bytes(1000, 6, 2)]
    elif name == "polish_only":
        assert want["ORDER"] == [0] and want["CLASS"] == [(0,) * 6] * 3 and want["WSBYTES"] == [0] and want["PAIRS"]
    elif name.startswith("err_"):
        assert want["rc"] == INVALID_ARG and want["msg"]
    elif name == "post_stride_spares_empty_chunks":
        assert want["rc"] == 0
    elif name == "refusals":
        assert want["PAIRS"] and want["MAXIMA"][4]
        assert [w[0] for w in want["WAVES"]] == [UNSUPPORTED] * 5 + [0]
        assert [w[1].split()[-1] for w in want["WAVES"][:5]] == ["phmm_pair_kernel", "phmm_wide_kernel", "phmm_kernel", "phmm_pair_kernel", "phmm_wide_kernel"]
    else:
        raise AssertionError("a case without its arm check: " + name)


def test_argument_errors_by_status_and_message(program_output):
    cases, got = program_output
    seen = {name: parse_batch(got[name]) for name in BATCH_NAMES if name.startswith("err_")}
    assert seen == {"err_not_contiguous": dict(rc=INVALID_ARG, msg="chunks must list their reads contiguously in order"),
                    "err_post_stride": dict(rc=INVALID_ARG, msg="post_stride smaller than a chunk's copy_num"),
                    "err_post_stride_sub_problem": dict(rc=INVALID_ARG, msg="post_stride smaller than a chunk's copy_num")}


@pytest.mark.parametrize("name", [c[0] for c in FEATURE_CASES])
def test_feature_chain_plan_matches_the_restatement(program_output, name):
    _, got = program_output
    (max_k, chunks), = [(k, c) for n, k, c in FEATURE_CASES if n == name]
    want = restate_features(max_k, chunks)
    evicted = want.pop("evicted")
    have = {tag: [int(x) for x in rows[0].split()] for tag, rows in got[name].items()}
    assert have == want
    if name == "features_evict":
        # three chunks that fit a CU's LDS one by one and not together: the largest by reads x columns leaves, then the next
        assert all(lds_bytes(*d) <= KIB160 for d in ((1000, 2, 2), (300, 21, 7), (1023, 10, 2), (1000, 2, 7))) and lds_bytes(1000, 21, 7) > KIB160
        assert evicted == [6, 2] and want["ORDER"] == [0, 3, 5, 1, 2, 4, 6] and want["LAUNCH"][:2] == [4, 3]   # failed between; in_ws sorted
        assert want["WSOFF"] == [0, ws_bytes(300, 21, 7), ws_bytes(300, 21, 7) + ws_bytes(1024, 1, 2)]
    elif name == "features_empty":
        assert want["ORDER"] == [] and want["LAUNCH"] == [0, 0, 1, 1, 2, 1, 1, 2]
    else:
        assert evicted == [] and want["LAUNCH"][:2] == [3, 0]


def test_chain_dims_of_a_chunk(program_output):
    _, got = program_output
    assert got["DIMS"] == [(copy,) + chain_dims(copy, 10 + copy) for copy in range(10)]
    assert {d for _, _, d, _ in got["DIMS"]} == {6, 9, 12, 15, 18, 21} and {k for _, _, _, k in got["DIMS"]} == {2, 3, 4, 5, 6, 7}


def test_which_filter_a_pass_takes(program_output):
    """batch_needs_tables, the dispatch of session_run between the fused filter and the table filter: the fused one counts in
    16-bit fields, so it is taken up to 65,535 reads of the deepest pile-up and not at 65,536; window polishing always has tables"""
    _, got = program_output
    assert got["TABLES"] == [(0, 0, 0), (0, 1, 0), (0, 65535, 0), (0, 65536, 1), (0, 0xffffffff, 1),
                             (1, 0, 1), (1, 1, 1), (1, 65535, 1), (1, 65536, 1), (1, 0xffffffff, 1)]
