// sum_final_body.h -- the body of sum_final_kernel, included INSIDE a kernel (phmm_kernels.hip; see band_prep_body.h for why).
// In: reads, chunks, state, hmm2, raw_all, rawG_all, lk_all, total_all; JTK_BODY_BLOCK = the chunk (blockIdx.y of a single launch).
    __shared__ __align__(16) double s_raw[FIN_ROWS * FIN_PITCH];
    __shared__ int s_G[FIN_ROWS];
    const uint32_t ci = JTK_BODY_BLOCK;
    const ChunkState st = state[ci];
    if (st.status != 0 || !st.active) return;
    const ChunkMeta cm = chunks[ci];
    const int L = (int)st.tmpl_len;
    const int p0 = (int)blockIdx.x * FIN_TILE;
    if (p0 > L) return;
    const int tid = threadIdx.x, p = p0 + tid;
    const int n_rows = min(FIN_ROWS, L + 1 - p0);
    double eMf[16], eMr[16];  // strand 1 -> hmm2[0], strand 0 -> hmm2[1] (as finalize_kernel)
#pragma unroll
    for (int k = 0; k < 16; k++) {
        eMf[k] = hmm2[0].eM[k];
        eMr[k] = hmm2[1].eM[k];
    }
    double tot[JTK_NUM_ROW];
#pragma unroll
    for (int k = 0; k < JTK_NUM_ROW; k++) tot[k] = 0.0;
    const uint32_t voters = (cm.take_num && cm.take_num < cm.n_reads) ? cm.take_num : cm.n_reads;
    for (uint32_t r = 0; r < voters; r++) {
        const uint32_t item = cm.read_first + r;
        const ReadMeta rm = reads[item];
        const double lk = lk_all[item];
        const bool dead = !(lk > JTK_LOG_ZERO);
        fin_stage(s_raw, s_G, raw_all + rm.raw_off, rawG_all + rm.row_off, p0, n_rows, tid, dead);
        __syncthreads();
        double res[JTK_NUM_ROW];
        if (rm.strand)
            fin_position(s_raw, s_G, eMf, tid, p, L, lk, dead, res);
        else
            fin_position(s_raw, s_G, eMr, tid, p, L, lk, dead, res);
#pragma unroll
        for (int k = 0; k < JTK_NUM_ROW; k++) tot[k] += res[k];
        __syncthreads();  // before the next read's rows are staged
    }
    if (p <= L) {
        double *total = total_all + cm.total_off + (uint64_t)p * JTK_NUM_ROW;
#pragma unroll
        for (int k = 0; k < JTK_NUM_ROW; k++) total[k] = tot[k];
    }
