// Source generator of the run-time compiled expression kernels
// (csrc/zxp_jit_source.cpp): a compiled ZXP program in, the kernel's HIP source
// and its input tables out.  Plain host C++, no HIP (the library and
// tests/cpp/jit_source_check.cpp link it).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/zkgpu.h"
#include "gl_host.hpp"

namespace zk {

struct ZxpJitIn {
    const zxp_instr *ins;  // compiled program (zkgpu_zxp_compile)
    uint32_t n_instr;
    const zxp_operand *opnd;
    uint32_t n_opnd;
    const zxp_term *terms;
    const uint64_t *csts;
    uint32_t n_tmp1, n_tmp3;
    const zkgpu_sections *sections;
    uint32_t log_dom;   // rows evaluated
    uint32_t log_omega; // x_i = x_start * omega_{2^log_omega}^i
    uint32_t wrap;      // shifted reads wrap mod 2^log_dom (else halo rows follow)
    const uint64_t *challenges, *publics, *evals;  // host
    const uint64_t *xdiv, *xdivw, *zh_dev;         // device
    uint32_t zmask;
    uint64_t x_start;
    double bytes;
    uint32_t dot_loop_min;  // DOTs with at least this many column terms loop over a table
    uint32_t waves_per_eu;  // occupancy hint for the compiler (0: none)
    uint32_t force_split;   // code blocks / limb chunks even below the size threshold (segments)
    const uint64_t *scratch;  // columns of section ZXP_SEC_SCRATCH (segments, csrc/zxp_segment.hpp)
    uint64_t scratch_ld;
};

// The launch settings of a whole program, for zkgpu_zxp_eval_dev and
// zkgpu_zxp_jit_source alike (the sources, and so the cache keys, match); a
// segment then sets force_split, its occupancy and scratch.
inline void zxp_jit_launch_settings(ZxpJitIn &in)
{
    in.dot_loop_min = 8;
    in.waves_per_eu = 0;
    in.force_split = 0;
    in.scratch = nullptr;
    in.scratch_ld = 0;
}

// A compiled program with these settings: all the source depends on.  The
// rest (domain, device tables, x_start, bytes) is zero for the launch to fill.
inline ZxpJitIn zxp_jit_in(const zxp_compiled &cp, const zkgpu_sections *sections, const uint64_t *challenges,
                           const uint64_t *publics, const uint64_t *evals)
{
    ZxpJitIn in{};
    in.ins = cp.instr;
    in.n_instr = cp.n_instr;
    in.opnd = cp.opnd;
    in.n_opnd = cp.n_opnd;
    in.terms = cp.term;
    in.csts = cp.cst;
    in.n_tmp1 = cp.n_tmp1;
    in.n_tmp3 = cp.n_tmp3;
    in.sections = sections;
    in.challenges = challenges;
    in.publics = publics;
    in.evals = evals;
    zxp_jit_launch_settings(in);
    return in;
}

// Dot3 limbs of a canonical coefficient c: 22/21/21-bit limbs of c and of
// c * 2^32 mod p (csrc/gl_device.hpp Dot3::term)
inline void zxp_limbs6(uint64_t c, uint32_t out[6])
{
    const uint64_t v[2] = {c, h_mul(c, 1ULL << 32)};
    for (int h = 0; h < 2; h++) {
        out[3 * h] = (uint32_t)(v[h] & ((1u << 22) - 1));
        out[3 * h + 1] = (uint32_t)((v[h] >> 22) & ((1u << 21) - 1));
        out[3 * h + 2] = (uint32_t)(v[h] >> 43);
    }
}

// column term of a looped DOT (device table; the kernel head declares the same layout)
struct JitTerm {
    const uint64_t *ptr;
    int64_t sh;
    uint32_t c[3][6];
    uint32_t pad[2];
};
static_assert(sizeof(JitTerm) == 96, "JitTerm");
// Shared with zxp_jit.hip only for the launch (jit_kl_lds: a table of nkl limb words is staged whole in LDS, programs
// that are not split) and the occupancy decisions (seg_ab: the segments' A/B switch ZKGPU_ZXP_SEG_AB, read once)
bool jit_kl_lds(size_t nkl);
struct SegAb {
    uint32_t waves = 0, slots = 0, prefetch = 0, block = 0, dist = 0;  // block / dist: 0 = the default
};
const SegAb &seg_ab();

// one kernel's source and input tables
struct ZxpJitSource {
    std::string src;
    std::vector<const uint64_t *> cp;  // column base pointers (slot j)
    std::vector<uint64_t> kc;          // F_p / F_p^3 constants
    std::vector<uint32_t> kl;          // DOT limbs (unrolled terms)
    std::vector<JitTerm> zt;           // DOT column terms (looped)
    bool split = false;                // code blocks and limb chunks (ZKJIT_SPLIT, ZKJIT_KL_CHUNK)
};

// 0 and `out` filled, or 1: unsupported program shape (the interpreter runs it)
int zxp_jit_build_source(const ZxpJitIn &in, ZxpJitSource &out);

}  // namespace zk
