// Host-side scalar Goldilocks (csrc/gl_host.cpp) and the twiddle-table shape:
// setup values only, all bulk math is on the GPU.  Plain host C++.
#pragma once
#include <cstdint>

namespace zk {

constexpr uint32_t TW_MAX_LOG = 28;  // big-twiddle base omega_{2^28}
constexpr uint32_t TW_LEVEL_BITS = 14;
constexpr uint64_t TW_LEVEL_SIZE = 1ULL << TW_LEVEL_BITS;

constexpr uint64_t HP = 0xFFFFFFFF00000001ULL;
inline uint64_t h_add(uint64_t a, uint64_t b)  // a, b < p
{
    const uint64_t s = a + b;
    return (s < a || s >= HP) ? s - HP : s;
}
uint64_t h_mul(uint64_t a, uint64_t b);
uint64_t h_pow(uint64_t a, uint64_t e);
uint64_t h_inv(uint64_t a);
uint64_t h_w(uint32_t n);

}  // namespace zk
