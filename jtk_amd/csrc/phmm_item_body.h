// phmm_item_body.h -- one item of phmm_kernel's work queue (read `item` of the session: both sweeps, unless the read has no part
// in this launch), included INSIDE the kernels' ticket loops (phmm_sweep.hip; see band_prep_body.h for why).  In: item, reads,
// chunks, state, bufs, ey_all, delta_all, hmm2, scratch, raw_all, rawG_all, lk_all, lds_tmpl, lds_read, only_active,
// skip_le_radius.
        const ReadMeta rm = reads[item];
        const ChunkMeta cm = chunks[rm.chunk];
        const ChunkState st = state[rm.chunk];
        if (st.status != 0) continue;
        if (only_active && !st.active) continue;
        if (cm.take_num && item - cm.read_first >= cm.take_num) continue;  // this read does not vote
        if (cm.radius > JTK_MAX_RADIUS) continue;                          // phmm_wide_kernel's read
        if (cm.radius <= skip_le_radius) continue;                         // phmm_pair_kernel's read
        const uint64_t *delta = delta_all + rm.delta_off;
        // the interval of diagonals whose whole band lies inside the DP matrix (band_prep_kernel)
        const uint64_t fastw = delta[((cm.tmpl_cap + rm.read_len) >> 6) + 2];
        // everything below was loaded through the vector memory path: make it scalar again (it is the same in every lane),
        // or the sweeps' control flow and addressing would be per-lane
        const int strand = uni((int)rm.strand), buf = uni((int)st.buf);
        sweep_read(uni((int)st.tmpl_len), uni((int)rm.read_len), uni((int)cm.radius), uni((int)(uint32_t)fastw),
                   uni((int)(uint32_t)(fastw >> 32)), hmm2 + (strand ? 0 : 1), bufs.tmpl[buf] + uni64(cm.tmpl_off),
                   ey_all + uni64(rm.ey_off), delta_all + uni64(rm.delta_off), scratch, raw_all + uni64(rm.raw_off),
                   rawG_all + uni64(rm.row_off), lk_all + item, lds_tmpl, lds_read);
