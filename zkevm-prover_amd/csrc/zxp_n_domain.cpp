// A quotient program (step42ns) re-targeted to the trace domain
// (zkgpu_zxp_to_n_domain, include/zkgpu.h): the constraint combination the
// program forms before its final "x ZI" vanishes on <omega_n> exactly when
// every polynomial identity holds on every row (with overwhelming probability
// over the combination challenge), so the same instruction list over the
// n-domain sections, without the division by Z_H, is a check of the trace.
// Only the operand table changes.  Plain host C++, no HIP: the library and
// tests/cpp/zxp_n_domain_check.cpp link it.
#include <cstdint>
#include <vector>

#include "../../include/zkgpu.h"
#include "../../include/zkgpu_zxp.h"

namespace zk {
int set_error(int code, const char *fmt, ...);  // api.hip
}

extern "C" int zkgpu_zxp_to_n_domain(zxp_operand *opnd_out, const zxp_instr *instr, uint32_t n_instr,
                                     const zxp_operand *opnd, uint32_t n_opnd, uint32_t extend_bits)
{
    using zk::set_error;
    if (!opnd_out || (n_instr && !instr) || (n_opnd && !opnd))
        return set_error(ZKGPU_ERR_ARG, "zxp_to_n_domain: null argument");
    if (extend_bits > 6) return set_error(ZKGPU_ERR_ARG, "zxp_to_n_domain: extend bits > 6");
    // how every operand is used: as a source, as a destination, and whether
    // every source use is a factor of a product stored to a q column
    std::vector<uint8_t> is_src(n_opnd, 0), is_dst(n_opnd, 0);
    auto q_col = [&](uint32_t k) {
        return (opnd[k].kind == ZXP_COL || opnd[k].kind == ZXP_COL3) && opnd[k].a == SEC_Q_2NS;
    };
    for (uint32_t k = 0; k < n_instr; k++) {
        const zxp_instr &I = instr[k];
        if (I.op > ZXP_COPY || I.dst >= n_opnd || I.a >= n_opnd || (I.op != ZXP_COPY && I.b >= n_opnd))
            return set_error(ZKGPU_ERR_ARG, "zxp_to_n_domain: instruction %u out of range", k);
        is_dst[I.dst] = 1;
        is_src[I.a] = 1;
        if (I.op != ZXP_COPY) is_src[I.b] = 1;
    }
    uint32_t n_zi_mul = 0;
    for (uint32_t k = 0; k < n_instr; k++) {
        const zxp_instr &I = instr[k];
        const bool za = opnd[I.a].kind == ZXP_ZI, zb = I.op != ZXP_COPY && opnd[I.b].kind == ZXP_ZI;
        if (opnd[I.dst].kind == ZXP_ZI)
            return set_error(ZKGPU_ERR_ARG, "zxp_to_n_domain: instruction %u writes ZI", k);
        if (!za && !zb) continue;
        // C x ZI -> q is the one place where dropping ZI keeps "zero iff satisfied"
        if (I.op != ZXP_MUL || !q_col(I.dst) || (za && zb))
            return set_error(ZKGPU_ERR_ARG,
                             "zxp_to_n_domain: instruction %u uses ZI other than as a factor of a product stored to "
                             "SEC_Q_2NS",
                             k);
        n_zi_mul++;
    }
    if (!n_zi_mul)
        return set_error(ZKGPU_ERR_ARG, "zxp_to_n_domain: no product by ZI is stored to SEC_Q_2NS: not a quotient program");
    static const uint32_t to_n[SEC_COUNT] = {0, 0, 0, 0, 0, SEC_CM1_N, SEC_CM2_N, SEC_CM3_N, 0, SEC_CONST_N, 0, 0};
    const int64_t step = 1LL << extend_bits;
    for (uint32_t k = 0; k < n_opnd; k++) {
        zxp_operand o = opnd[k];
        switch (o.kind) {
        case ZXP_TMP1:
        case ZXP_TMP3:
        case ZXP_LIT:
        case ZXP_CHAL:
        case ZXP_PUB:
        case ZXP_X: break;
        case ZXP_ZI: o = zxp_operand{ZXP_LIT, 1, 0, 0}; break;
        case ZXP_COL:
        case ZXP_COL3: {
            const int64_t sh = (int32_t)o.c;
            if (o.a == SEC_Q_2NS) {
                if (is_src[k]) return set_error(ZKGPU_ERR_ARG, "zxp_to_n_domain: operand %u reads SEC_Q_2NS", k);
                if (sh) return set_error(ZKGPU_ERR_ARG, "zxp_to_n_domain: operand %u stores to SEC_Q_2NS at row shift %d", k, (int)sh);
                break;
            }
            if (o.a != SEC_CM1_2NS && o.a != SEC_CM2_2NS && o.a != SEC_CM3_2NS && o.a != SEC_CONST_2NS)
                return set_error(ZKGPU_ERR_ARG, "zxp_to_n_domain: operand %u names section %u", k, o.a);
            if (is_dst[k]) return set_error(ZKGPU_ERR_ARG, "zxp_to_n_domain: operand %u stores to section %u", k, o.a);
            if (sh % step)
                return set_error(ZKGPU_ERR_ARG, "zxp_to_n_domain: operand %u: row shift %d is no multiple of %d", k,
                                 (int)sh, (int)step);
            o.a = to_n[o.a];
            o.c = (uint32_t)(int32_t)(sh / step);
            break;
        }
        default: return set_error(ZKGPU_ERR_ARG, "zxp_to_n_domain: operand %u of kind %u", k, o.kind);
        }
        opnd_out[k] = o;
    }
    return 0;
}
