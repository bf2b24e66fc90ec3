// chain_jump_table.h -- included by mcmc_kernels.hip alone: the host builder of the producer's jump table and its upload.
#pragma once
#include <mutex>
#include <vector>

// ---- host: the byte-digit table of M^(63*SEG), from nothing but the generator's own step function
namespace {
struct V256 {
    uint64_t w[4];
};
V256 host_xo_step(V256 v) {
    uint64_t s0 = v.w[0], s1 = v.w[1], s2 = v.w[2], s3 = v.w[3];
    const uint64_t t = s1 << 17;
    s2 ^= s0;
    s3 ^= s1;
    s1 ^= s2;
    s0 ^= s3;
    s2 ^= t;
    s3 = (s3 << 45) | (s3 >> 19);
    return V256{{s0, s1, s2, s3}};
}
struct M256 {
    V256 col[256];  // image of unit vector b (bit b & 63 of word b >> 6)
};
V256 m_apply(const M256 &a, const V256 &v) {
    V256 r{{0, 0, 0, 0}};
    for (int b = 0; b < 256; b++)
        if ((v.w[b >> 6] >> (b & 63)) & 1ull)
            for (int q = 0; q < 4; q++) r.w[q] ^= a.col[b].w[q];
    return r;
}
void m_mul(const M256 &a, const M256 &b, M256 &out) {  // out = a * b
    for (int i = 0; i < 256; i++) out.col[i] = m_apply(a, b.col[i]);
}
std::vector<uint64_t> build_jump_table(uint32_t SEG) {
    std::vector<uint64_t> tab;
    auto *m = new M256, *acc = new M256, *tmp = new M256;
    for (int b = 0; b < 256; b++) {
        V256 e{{0, 0, 0, 0}};
        e.w[b >> 6] = 1ull << (b & 63);
        m->col[b] = host_xo_step(e);
        acc->col[b] = e;  // identity
    }
    for (uint32_t e = 63u * SEG; e; e >>= 1) {  // acc = M^(63*SEG) by square and multiply
        if (e & 1u) {
            m_mul(*m, *acc, *tmp);
            *acc = *tmp;
        }
        m_mul(*m, *m, *tmp);
        *m = *tmp;
    }
    tab.resize((size_t)32 * 256 * 4);
    for (int k = 0; k < 32; k++)
        for (int v = 0; v < 256; v++) {
            V256 x{{0, 0, 0, 0}};
            x.w[k >> 3] = (uint64_t)v << (8 * (k & 7));
            const V256 r = m_apply(*acc, x);
            for (int q = 0; q < 4; q++) tab[((size_t)k * 256 + v) * 4 + q] = r.w[q];
        }
    delete m;
    delete acc;
    delete tmp;
    return tab;
}
const std::vector<uint64_t> &jump_table_host() {  // sessions run on several host threads: initialised exactly once
    static const std::vector<uint64_t> tab = [] {  // [seg_log - 3]: the tables of M^(63 * 8) and M^(63 * 16), back to back
        std::vector<uint64_t> t = build_jump_table(1u << JTK_SEG_LOG_GENERAL);
        const std::vector<uint64_t> u = build_jump_table(1u << JTK_SEG_LOG_LIGHT);
        t.insert(t.end(), u.begin(), u.end());
        return t;
    }();
    return tab;
}
std::mutex g_jump_mutex;
bool g_jump_uploaded[64];  // per device ordinal

// The table is a constant of the generator: uploaded once per device, synchronously, before the first chain kernel.
int mcmc_upload_jump_table() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return -1;
    std::lock_guard<std::mutex> lock(g_jump_mutex);
    if (g_jump_uploaded[dev]) return 0;
    const std::vector<uint64_t> &tab = jump_table_host();
    const hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(g_jump_tab), tab.data(), tab.size() * 8, 0, hipMemcpyHostToDevice);
    if (e == hipSuccess) g_jump_uploaded[dev] = true;
    return (int)e;
}
}  // namespace
