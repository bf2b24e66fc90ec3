// band_prep_body.h -- the body of band_prep_kernel, included INSIDE a kernel (phmm_kernels.hip): once in the single-session
// kernel, whose parameters it names, and once in band_prep_merged_kernel, which binds the same names to a segment of its table.
// Textual inclusion and not a __device__ function: the single-session kernel has to stay the machine code it was, and an inlined
// body is scheduled differently.  In: n_reads, reads, chunks, state, bufs, delta, only_active, max_words; JTK_BODY_BLOCK = the
// workgroup's index among the session's.
    extern __shared__ __align__(8) unsigned char bp_smem[];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t r = JTK_BODY_BLOCK * BP_WAVES + wave;
    if (r >= n_reads) return;
    const ReadMeta rm = reads[r];
    ChunkState *st = &state[rm.chunk];
    if (st->status != 0) return;
    if (only_active && !st->active) return;
    unsigned long long *sd = reinterpret_cast<unsigned long long *>(bp_smem) + (size_t)wave * max_words;
    const uint32_t L = st->tmpl_len, n = rm.read_len, T = L + n;
    const uint8_t *ops = bufs.ops[st->buf] + rm.ops_off;
    const uint32_t n_ops = bufs.ops_len[st->buf][r];
    uint64_t *d = delta + rm.delta_off;
    const uint32_t words = (T >> 6) + 2;
    for (uint32_t w = lane; w < words; w += 64) sd[w] = 0ull;
    // the interval [f_lo, f_hi] of diagonals whose WHOLE band lies inside the DP matrix (0 <= i <= L, 0 <= j <= n for every
    // band cell): c - r >= 0, c + r <= L, c + r <= t, c - r >= t - n.  c and t - c are non-decreasing in t, so the set is one
    // interval; phmm_kernel runs it under an EXEC mask that is the band and takes per-lane predicates outside of it.
    const int32_t rad = (int32_t)chunks[rm.chunk].radius;
    uint32_t f_lo = 0xffffffffu, f_hi = 0;  // per lane: min / max of the diagonals it saw satisfy the condition
    auto visit = [&](uint32_t tt, uint32_t cc) {  // diagonal tt has centre cc
        const int32_t c = (int32_t)cc, td = (int32_t)tt;
        if (c - rad >= 0 && c + rad <= (int32_t)L && c + rad <= td && c - rad >= td - (int32_t)n) {
            f_lo = tt < f_lo ? tt : f_lo;
            f_hi = tt > f_hi ? tt : f_hi;
        }
    };
    uint32_t i0 = 0, j0 = 0;  // template / read bases consumed before this step's 64 ops (uniform)
    bool bad = false;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (uint32_t base = 0; base < n_ops && !bad; base += 64) {
        const uint32_t k = base + lane;
        const bool has = k < n_ops;
        const uint32_t op = has ? ops[k] : (uint32_t)JTK_OP_INS;
        const bool invalid = has && op > JTK_OP_DEL;
        const bool di = has && (op <= JTK_OP_MISMATCH || op == JTK_OP_DEL), dj = has && (op <= JTK_OP_MISMATCH || op == JTK_OP_INS);
        const unsigned long long mi = __ballot(di), mj = __ballot(dj);
        const uint32_t i = i0 + (uint32_t)__popcll(mi & below), j = j0 + (uint32_t)__popcll(mj & below), t = i + j;  // before the op
        const uint32_t t_after = t + (di ? 1u : 0u) + (dj ? 1u : 0u);
        // (the serial walk stopped at the first op that passed diagonal T: nothing behind it left a bit or a visit; the read is
        // bad either way, and so is its chunk -- only the bounds matter here)
        if (has && !invalid && t_after <= T + 2) {
            if (op == JTK_OP_INS) {
                visit(t + 1, i);
            } else {
                if (t + 1 <= T) atomicOr(&sd[(t + 1) >> 6], 1ull << ((t + 1) & 63u));
                visit(t + 1, i + 1);
                if (op != JTK_OP_DEL) visit(t + 2, i + 1);
            }
        }
        if (__ballot(invalid || (has && t_after > T)) != 0ull) bad = true;
        i0 += (uint32_t)__popcll(mi);
        j0 += (uint32_t)__popcll(mj);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t a = __shfl_xor(f_lo, o, 64), b = __shfl_xor(f_hi, o, 64);
        f_lo = a < f_lo ? a : f_lo;
        f_hi = b > f_hi ? b : f_hi;
    }
    if (bad || i0 != L || j0 != n) {
        bad = true;
        if (lane == 0) atomicMin(&st->status, (int)JTK_ERR_OPS_MISMATCH);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // the wave's own LDS atomics are done before its lanes read the words
    for (uint32_t w = lane; w < words; w += 64) d[w] = sd[w];
    // the word behind the read's delta words (session.hip sizes the slot from the template CAPACITY: one word to spare)
    if (lane == 0)
        d[((chunks[rm.chunk].tmpl_cap + rm.read_len) >> 6) + 2] = (bad || f_hi < f_lo) ? 1ull : ((uint64_t)f_hi << 32 | f_lo);
