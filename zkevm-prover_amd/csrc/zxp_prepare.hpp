// Host side of zkgpu_zxp_eval_dev / zkgpu_zxp_eval_block_dev
// (csrc/zxp_prepare.cpp): the argument checks, the plan (compile or slot
// packing, zhInv, path choice) and the interpreter's records.  Plain host C++,
// no HIP (the library and tests/cpp/zxp_prepare_check.cpp link it); api.hip
// keeps the tables on the device, the uploads and the launches.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/zkgpu.h"
#include "../../include/zkgpu_zxp.h"

namespace zk {

// Pre-decoded ZXP instruction of the interpreter (k_zxp_eval, stark.hip): every
// operand is resolved to a source kind plus a ready pointer / shift / stride /
// immediate, so the kernel fetches one 128-byte record per instruction with
// wave-uniform scalar loads and no dependent descriptor or section lookups.
enum { DK_T1 = 0, DK_T3, DK_C1, DK_C3, DK_IMM1, DK_IMM3, DK_X, DK_I3, DK_ZI };
struct alignas(16) ZOp {
    uint32_t op, ka, kb, kd;
    const uint64_t *pa, *pb;
    uint64_t *pd;
    int32_t ia, ib, id;  // T*: slot offset (slot * 64); C*: row shift; ZI: index mask
                         // DOT: ia = first term, ib = term count; ima/imb = constant limbs (9 u32)
    uint32_t lda, ldb, ldd;
    uint64_t ima[3], imb[3];
    uint64_t pad[2];
};
static_assert(sizeof(ZOp) == 128, "ZOp is two 64-byte scalar loads");

// ZXP_DOT term: source (a column at a row shift, or an LDS temp slot
// component) and its F_p^3 coefficient as Dot3 limbs (3 components x 6).
struct alignas(16) ZTerm {
    uint32_t kind;  // DK_C1 or DK_T1
    int32_t ii;     // C1: row shift; T1: LDS offset (slot * 64)
    const uint64_t *ptr;
    uint32_t c[3][6];
    uint32_t pad[2];
};
static_assert(sizeof(ZTerm) == 96, "ZTerm is 96 bytes");

// the interpreter's launch (zxp_eval, stark.hip)
struct ZxpLaunch {
    const ZOp *prog;     // device, n_instr records
    const ZTerm *terms;  // device, DOT terms
    uint32_t n_instr, n_tmp1, n_tmp3;
    uint32_t logdom;    // rows evaluated
    uint32_t logomega;  // x_i = x_start * omega_{2^logomega}^i
    uint32_t wrap;      // shifted reads wrap mod 2^logdom (else halo rows follow)
    uint64_t x_start;
    double bytes;  // algorithmic bytes for profiling
};

// The arguments of one evaluation, as the two C-ABI entries take them.
// log_dom: rows evaluated (2^log_dom); log_omega: x_i = x_start * w_{2^log_omega}^i and zhInv's N =
// 2^(log_omega - extend_bits); wrap: shifted reads wrap mod 2^log_dom, else halo rows follow the block
struct ZxpArgs {
    const zxp_instr *instr;
    uint32_t n_instr;
    const zxp_operand *opnd;
    uint32_t n_opnd;
    uint32_t n_tmp1, n_tmp3;
    const zkgpu_sections *sections;
    uint32_t log_dom, log_omega;
    int wrap;
    const uint64_t *challenges, *publics;
    uint32_t n_publics;
    const uint64_t *evals;
    uint32_t n_evals;
    const uint64_t *xdiv, *xdivw;  // device
    uint32_t extend_bits;
    uint64_t x_start;
    // zkgpu_zxp_eval_rows_dev: the program runs at rows[0 .. n_rows) (device) of the domain and its
    // stores are compact (index j of the destination for rows[j])
    bool row_list = false;
    const uint64_t *rows = nullptr;
    uint32_t n_rows = 0;
};
constexpr uint32_t ZXP_MAX_LIST_ROWS = 4096;

// What runs: the compiled program (its tables are the compiler's, valid on
// this thread until its next compile), or with ZKGPU_ZXP_FUSE=0 the source
// program over `packed`, its operand table with the temp slots packed.  One
// plan serves the compiled kernels and the interpreter.
struct ZxpPlan {
    zxp_compiled prog;
    std::vector<zxp_operand> packed;
    uint32_t n_dot_terms;  // DOT terms with a source: the interpreter's ZTerm records
    uint64_t zhinv[64];    // zhInv[j] = 1/(7^N * W[eb]^j - 1), j < n_zhinv (zhInv.cpp:7-31)
    uint32_t n_zhinv;
    bool uses_zi;  // the program has a ZI operand: else zhinv is zero and nothing reads it
    double bytes;  // algorithmic bytes: every distinct column operand read once per row + written columns
    bool jit;      // the run-time compiled kernels (csrc/zxp_jit.hip), else the interpreter
};

// Each phase returns 0, or an error code with the message in set_error.
// Every check of the caller's arguments, before anything is computed from them
int zxp_validate(const ZxpArgs &a);
// Reads ZKGPU_ZXP_FUSE, ZKGPU_ZXP_MAX_TERMS and ZKGPU_ZXP_JIT (on every call)
int zxp_plan(const ZxpArgs &a, ZxpPlan &p);
// The interpreter's records; zh_dev: device address of p.zhinv.  Also the
// interpreter's own bound: its temporaries live in LDS
int zxp_records(const ZxpArgs &a, const ZxpPlan &p, const uint64_t *zh_dev, std::vector<ZOp> &ops,
                std::vector<ZTerm> &terms);

}  // namespace zk
