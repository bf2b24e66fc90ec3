// chain_stats.h -- included by mcmc_kernels.hip alone: everything that depends on JTK_MCMC_STATS, the statistics build of the
// chains (build.build_experiment, scripts/chain_pieces.py): cycle counters and printf rows the product compiles none of.
#pragma once

#ifdef JTK_MCMC_STATS
#define JTK_STAT(...) __VA_ARGS__  // a statement or declaration of the statistics build only
// mcmc_chain: GS_MARK(k) adds the time since the last mark to gs[k] (gs_t: the step's stopwatch)
#define GS_MARK(k) { const unsigned long long now_ = __builtin_readcyclecounter(); gs[k] += now_ - gs_t; gs_t = now_; }
// mcmc_chain_tab
#define TS_ADD(k, v) ts[k] += (v)
// mcmc_chain_k2: counters live in scalar registers during the chain and are folded into LDS once per chain
#define ST_T0() unsigned long long st_acc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; unsigned long long st_mk = 0; (void)st_mk; const unsigned long long st_t0 = __builtin_readcyclecounter()
#define ST_ADD(k) st_acc[k] += __builtin_readcyclecounter() - st_t0; if (lane == 0) { for (int q_ = 0; q_ < 16; q_++) m.k2_stats[q_] += st_acc[q_]; }
#define ST_CNT(k, v) st_acc[k] += (v)
// the pieces of an event: ST_MARK0 starts the stopwatch, ST_MARK(k) adds the time since the last mark to counter k
#define ST_MARK0() st_mk = __builtin_readcyclecounter()
#define ST_MARK(k) { const unsigned long long now_ = __builtin_readcyclecounter(); st_acc[k] += now_ - st_mk; st_mk = now_; }
#else
#define JTK_STAT(...)
#define GS_MARK(k)
#define TS_ADD(k, v)
#define ST_T0()
#define ST_ADD(k)
#define ST_CNT(k, v)
#define ST_MARK0()
#define ST_MARK(k)
#endif
