// rethread_body.h -- the body of rethread_kernel, included INSIDE a kernel (polish_kernels.hip; see band_prep_body.h for why).
// In: n_reads, reads, chunks, state, bufs, ey_all, edits_all; JTK_BODY_BLOCK = the workgroup's index among the session's.
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t r = JTK_BODY_BLOCK * RT_WAVES + (threadIdx.x >> 6);
    if (r >= n_reads) return;
    const ReadMeta rm = reads[r];
    ChunkState *st = &state[rm.chunk];
    if (st->status != 0 || !st->active || st->n_edits == 0) return;
    const ChunkMeta cm = chunks[rm.chunk];
    const uint32_t L = st->tmpl_len, ne = st->n_edits, b = st->buf, nb = JTK_NEXT_BUF(b);
    const Edit *edits = edits_all + cm.edit_off;
    const uint8_t *ops = bufs.ops[b] + rm.ops_off;
    uint8_t *out = bufs.ops[nb] + rm.ops_off;
    const uint32_t n_ops = bufs.ops_len[b][r];
    const uint8_t *tmpl = bufs.tmpl[nb] + cm.tmpl_off;  // the edited template
    const uint8_t *ey = ey_all + rm.ey_off;               // read base j is ey[j+1] & 3
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t w0 = 0, ti0 = 0, ni0 = 0, nj0 = 0;  // uniform: ops written, old template bases consumed, new template / read position
    uint32_t e_cur = 0;                          // uniform: edits before it cannot touch an op from here on
    bool overflow = false;
    // an insertion edit at position 0 fires before the first op
    if (edits[0].pos == 0 && edits[0].row >= 4 && edits[0].row < 11) {
        const uint32_t k = edit_inserted(edits[0].row, 0, L);
        if (lane < k && lane < rm.ops_cap) out[lane] = JTK_OP_DEL;
        overflow = overflow || k > rm.ops_cap;
        w0 = k;
        ni0 = k;
    }
    for (uint32_t base = 0; base < n_ops; base += 64) {
        const uint32_t kk = base + lane;
        const bool has = kk < n_ops;
        const uint32_t op = has ? ops[kk] : (uint32_t)JTK_OP_INS;
        const bool cons = has && op != JTK_OP_INS;                   // consumes an old template base
        const unsigned long long mc = __ballot(cons);
        const uint32_t ti = ti0 + (uint32_t)__popcll(mc & below);    // old bases consumed before this op
        // edits whose reach ends before this step's first consuming op are behind us (uniform cursor)
        while (e_cur < ne) {
            const Edit ed = edits[e_cur];
            const uint32_t last = ed.row >= 11 ? ed.pos + (ed.row - 10) - 1 : (ed.row >= 4 ? ed.pos - 1 : ed.pos);  // last ti it touches
            if ((ed.row >= 4 && ed.row < 11 && ed.pos == 0) || last < ti0)
                e_cur++;
            else
                break;
        }
        uint32_t first = has ? op : 4u;   // what the op becomes: an op code, or 4 = nothing
        uint32_t k_del = 0;               // Del ops that follow it
        if (cons) {
            for (uint32_t e = e_cur; e < ne; e++) {
                const Edit ed = edits[e];
                if (ed.pos > ti + 1) break;
                if (ed.row >= 11) {
                    if (ed.pos <= ti && ti < ed.pos + (ed.row - 10)) first = op != JTK_OP_DEL ? (uint32_t)JTK_OP_INS : 4u;
                } else if (ed.row >= 4 && ed.pos == ti + 1) {
                    k_del = edit_inserted(ed.row, ed.pos, L);
                }
            }
        }
        const uint32_t c_out = (first != 4u ? 1u : 0u) + k_del;
        const uint32_t c_t = ((first <= JTK_OP_MISMATCH || first == JTK_OP_DEL) ? 1u : 0u) + k_del;     // new template bases consumed
        const uint32_t c_r = (first <= JTK_OP_MISMATCH || first == JTK_OP_INS) ? 1u : 0u;                // read bases consumed
        const uint32_t packed = c_out | c_t << 10 | c_r << 20;
        uint32_t incl = packed;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u = __shfl_up(incl, o, 64);
            if ((int)lane >= o) incl += u;
        }
        const uint32_t excl = incl - packed, total = __shfl(incl, 63, 64);
        uint32_t w = w0 + (excl & 1023u);
        const uint32_t ni = ni0 + ((excl >> 10) & 1023u), nj = nj0 + (excl >> 20);
        if (first != 4u) {
            uint32_t o1 = first;
            if (first <= JTK_OP_MISMATCH) o1 = tmpl[ni] == (ey[nj + 1] & 3) ? JTK_OP_MATCH : JTK_OP_MISMATCH;
            if (w < rm.ops_cap) out[w] = (uint8_t)o1;
            w++;
        }
        for (uint32_t q = 0; q < k_del; q++)
            if (w + q < rm.ops_cap) out[w + q] = JTK_OP_DEL;
        w0 += total & 1023u;
        ni0 += (total >> 10) & 1023u;
        nj0 += total >> 20;
        ti0 += (uint32_t)__popcll(mc);
        overflow = overflow || w0 > rm.ops_cap;
    }
    if (lane == 0) {
        bufs.ops_len[nb][r] = overflow ? rm.ops_cap : w0;
        if (overflow) atomicMin(&st->status, (int)JTK_ERR_CHUNK_FAILED);
    }
