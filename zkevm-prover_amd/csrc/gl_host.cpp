// Host scalar field (setup constants only).
#include "gl_host.hpp"

namespace zk {

// (a b) mod p by the Goldilocks folding 2^64 = 2^32 - 1, 2^96 = -1 (no 128-bit
// division: the expression kernels' limb tables take ~10^5 of these per proof)
uint64_t h_mul(uint64_t a, uint64_t b)
{
    const unsigned __int128 x = (unsigned __int128)a * b;
    const uint64_t lo = (uint64_t)x, hi = (uint64_t)(x >> 64), eps = 0xFFFFFFFFULL;
    const uint64_t hh = hi >> 32, hl = hi & eps;
    uint64_t t0 = lo - hh;
    if (lo < hh) t0 -= eps;  // borrow: 2^64 == eps
    const uint64_t t1 = (hl << 32) - hl;
    uint64_t r = t0 + t1;
    if (r < t1) r += eps;  // carry: no second one
    return r >= HP ? r - HP : r;
}
uint64_t h_pow(uint64_t a, uint64_t e)
{
    uint64_t r = 1;
    a %= HP;
    while (e) {
        if (e & 1) r = h_mul(r, a);
        a = h_mul(a, a);
        e >>= 1;
    }
    return r;
}
uint64_t h_inv(uint64_t a) { return h_pow(a, HP - 2); }
uint64_t h_w(uint32_t n)
{
    uint64_t w = 7277203076849721926ULL;  // W[32]
    for (uint32_t i = n; i < 32; i++) w = h_mul(w, w);
    return w;
}

}  // namespace zk
