// The constraint combination of a quotient program (step42ns) taken apart into
// its terms (zkgpu_zxp_split_constraints, include/zkgpu.h).  The program folds
// its identities C_k into one value C with powers of the combination challenge
// alpha = CHAL[chal] and stores C (x ZI) to q; the split finds, without
// matching any instruction pattern, which values enter C at which power of
// alpha, and writes a TAPPED program that stores every such value v_k to its
// own F_p^3 column, so that per row
//     C = sum over live terms k of (-1)^negated_k * alpha^exponent_k * v_k.
//
// The rule.  Walk the instructions in order and track every temporary SLOT
// (kind + slot, not operand index).  A slot holds a PLAIN value (free of
// alpha) or a COMBINATION: a set of terms, each with a power of alpha and a
// sign.  Every operand that is no temporary is plain, but CHAL[chal]:
//   a read of CHAL[chal] itself (COPY, ADD, SUB source; the factor of a MUL
//   whose other factor is CHAL[chal] too)
//                          the combination {literal 1 . alpha^1}, a new term
//   MUL comb x CHAL[chal]  every exponent + 1
//   MUL plain x CHAL[chal] a new term x at exponent 1
//   ADD / SUB comb, plain x   x joins as a new term at exponent 0, negated when
//                          it is subtracted; plain - comb flips every term
//   ADD / SUB comb, comb   the union (the second negated by SUB); refused when
//                          they share a term
//   COPY comb              copies it
//   plain sources only     the instruction is kept verbatim, its destination
//                          slot becomes plain
//   MUL comb x anything else, into a TMP3 slot
//                          the slot is SPOILED (a value the rule does not
//                          follow), and so is the TMP3 destination of any
//                          instruction that reads a spoiled slot; such
//                          instructions are dropped.  The program is refused,
//                          naming the product's instruction, as soon as a
//                          spoiled value would count: read together with a
//                          combination or with CHAL[chal], or written anywhere
//                          but to a TMP3 slot.  A product that feeds nothing
//                          changes nothing in C.
// Terms are numbered in the order they join (within one instruction: the
// reads of CHAL[chal], first source first, then the plain values likewise).
// A combination may only be written to a TMP3 slot or, once, to
// COL3(SEC_Q_2NS, column 0, shift 0), and that by a COPY or by a MUL with ZI
// or the literal 1 (what zkgpu_zxp_to_n_domain leaves of ZI).  exponent and
// negated of a term are those it has in that stored value; a term that never
// reaches q is dead.  instr is the source instruction at which it joined.
//
// The tapped program: every instruction with a combination among its sources
// or as its result is dropped; where term k joins, COPY COL3(SEC_Q_2NS, 3k)
// <- x is emitted (a base value stored to a COL3 zeroes components 1 and 2).
// Its operand table is the source's, then in order of need one LIT 1 (the
// value of a read of CHAL[chal]) and one COL3(SEC_Q_2NS, 3k, 0) per term.
// Plain host C++, no HIP: the library and tests/cpp/zxp_split_check.cpp link it.
#include <cstdint>
#include <unordered_map>
#include <vector>

#include "../../include/zkgpu.h"
#include "../../include/zkgpu_zxp.h"

namespace zk {
int set_error(int code, const char *fmt, ...);  // api.hip
}

namespace {

struct Entry {
    uint32_t id, exponent, negated;
};
typedef std::vector<Entry> Comb;

}  // namespace

extern "C" int zkgpu_zxp_split_constraints(zxp_instr *instr_out, uint32_t *n_instr_out, zxp_operand *opnd_out,
                                           uint32_t *n_opnd_out, zxp_split_term *terms, uint32_t *n_terms,
                                           const zxp_instr *instr, uint32_t n_instr, const zxp_operand *opnd,
                                           uint32_t n_opnd, uint32_t chal)
{
    using zk::set_error;
    if (!instr_out || !n_instr_out || !opnd_out || !n_opnd_out || !terms || !n_terms || (n_instr && !instr) ||
        (n_opnd && !opnd))
        return set_error(ZKGPU_ERR_ARG, "zxp_split: null argument");
    if (chal >= 8) return set_error(ZKGPU_ERR_ARG, "zxp_split: challenge %u out of range", chal);
    if (n_instr > 0x20000000u) return set_error(ZKGPU_ERR_ARG, "zxp_split: too many instructions");
    uint32_t ni = 0, no = n_opnd, nt = 0;
    for (uint32_t k = 0; k < n_opnd; k++) opnd_out[k] = opnd[k];
    std::unordered_map<uint32_t, Comb> slots;  // TMP3 slot -> the combination it holds
    uint32_t lit1 = UINT32_MAX;                // operand index of the appended LIT 1
    std::vector<uint8_t> seen;                 // by term id, for the union's shared-term test
    Comb q;
    bool have_q = false;

    const auto is_alpha = [&](uint32_t o) { return opnd[o].kind == ZXP_CHAL && opnd[o].a == chal; };
    const auto comb_of = [&](uint32_t o) -> const Comb * {
        if (opnd[o].kind != ZXP_TMP3) return nullptr;
        const auto it = slots.find(opnd[o].a);
        return it == slots.end() ? nullptr : &it->second;
    };
    const auto is_one = [&](uint32_t o) {
        return opnd[o].kind == ZXP_ZI || (opnd[o].kind == ZXP_LIT && opnd[o].a == 1 && opnd[o].b == 0);
    };
    // TMP3 slot -> the instruction whose product of a combination by something other than alpha
    // (or a value derived from that product) it holds
    std::unordered_map<uint32_t, uint32_t> spoiled;
    const uint32_t NONE = UINT32_MAX;
    const auto spoiled_of = [&](uint32_t o) {
        if (opnd[o].kind != ZXP_TMP3) return NONE;
        const auto it = spoiled.find(opnd[o].a);
        return it == spoiled.end() ? NONE : it->second;
    };
    const auto not_alpha = [&](uint32_t k) {
        return set_error(ZKGPU_ERR_ARG,
                         "zxp_split: instruction %u multiplies a combination by something other than the "
                         "combination challenge",
                         k);
    };
    // term nt joins at instruction k with value x (an operand index, or UINT32_MAX: the literal 1)
    const auto join = [&](uint32_t k, uint32_t x) {
        if (x == UINT32_MAX) {
            if (lit1 == UINT32_MAX) {
                lit1 = no;
                opnd_out[no++] = zxp_operand{ZXP_LIT, 1, 0, 0};
            }
            x = lit1;
        }
        opnd_out[no] = zxp_operand{ZXP_COL3, SEC_Q_2NS, 3 * nt, 0};
        instr_out[ni++] = zxp_instr{ZXP_COPY, no++, x, 0};
        terms[nt] = zxp_split_term{0, 0, k, 1};
        return nt++;
    };

    for (uint32_t k = 0; k < n_instr; k++) {
        const zxp_instr &I = instr[k];
        if (I.op > ZXP_COPY || I.dst >= n_opnd || I.a >= n_opnd || (I.op != ZXP_COPY && I.b >= n_opnd))
            return set_error(ZKGPU_ERR_ARG, "zxp_split: instruction %u out of range", k);
        const zxp_operand &D = opnd[I.dst];
        // a source derived from a product the rule does not follow: only another such value
        // may come of it, in a TMP3 slot
        const uint32_t sa = spoiled_of(I.a), sb = I.op == ZXP_COPY ? NONE : spoiled_of(I.b);
        if (sa != NONE || sb != NONE) {
            const uint32_t from = sa != NONE ? sa : sb, other = sa != NONE ? I.b : I.a;
            if (D.kind != ZXP_TMP3 || (I.op != ZXP_COPY && (is_alpha(other) || comb_of(other)))) return not_alpha(from);
            slots.erase(D.a);
            spoiled[D.a] = from;
            continue;
        }
        Comb R;
        bool comb = false, q_form = false;  // q_form: a COPY, or a MUL by ZI or the literal 1
        if (I.op == ZXP_COPY) {
            if (is_alpha(I.a)) {
                R.push_back(Entry{join(k, UINT32_MAX), 1, 0});
                comb = true;
            } else if (const Comb *c = comb_of(I.a)) {
                R = *c;
                comb = true;
            }
            q_form = true;
        } else if (I.op == ZXP_MUL && (is_alpha(I.a) || is_alpha(I.b))) {
            const uint32_t other = is_alpha(I.b) ? I.a : I.b;
            if (is_alpha(other))
                R.push_back(Entry{join(k, UINT32_MAX), 2, 0});
            else if (const Comb *c = comb_of(other)) {
                R = *c;
                for (Entry &e : R) e.exponent++;
            } else
                R.push_back(Entry{join(k, other), 1, 0});
            comb = true;
        } else if (I.op == ZXP_MUL) {
            const Comb *ca = comb_of(I.a), *cb = comb_of(I.b);
            if (ca || cb) {
                if (D.kind == ZXP_TMP3) {  // refused only if it ever reaches a combination or a column
                    slots.erase(D.a);
                    spoiled[D.a] = k;
                    continue;
                }
                const bool to_q = (D.kind == ZXP_COL || D.kind == ZXP_COL3) && D.a == SEC_Q_2NS;
                if ((ca && cb) || !is_one(ca ? I.b : I.a) || !to_q) return not_alpha(k);
                R = ca ? *ca : *cb;
                comb = q_form = true;
            }
        } else {  // ADD, SUB
            const bool sub = I.op == ZXP_SUB;
            const Comb *ca = comb_of(I.a), *cb = comb_of(I.b);
            Comb fa, fb;  // a read of CHAL[chal] itself
            if (is_alpha(I.a)) fa.push_back(Entry{join(k, UINT32_MAX), 1, 0}), ca = &fa;
            if (is_alpha(I.b)) fb.push_back(Entry{join(k, UINT32_MAX), 1, 0}), cb = &fb;
            if (ca || cb) {
                comb = true;
                if (ca) R = *ca;
                if (cb) {
                    seen.assign(nt, 0);
                    for (const Entry &e : R) seen[e.id] = 1;
                    for (const Entry &e : *cb) {
                        if (seen[e.id])
                            return set_error(ZKGPU_ERR_ARG,
                                             "zxp_split: instruction %u combines two combinations that share term %u",
                                             k, e.id);
                        R.push_back(Entry{e.id, e.exponent, e.negated ^ (sub ? 1u : 0u)});
                    }
                }
                if (!ca) R.push_back(Entry{join(k, I.a), 0, 0});
                if (!cb) R.push_back(Entry{join(k, I.b), 0, sub ? 1u : 0u});
            }
        }
        const bool dst_q = (D.kind == ZXP_COL || D.kind == ZXP_COL3) && D.a == SEC_Q_2NS;
        if (!comb) {
            if (dst_q)
                return set_error(ZKGPU_ERR_ARG,
                                 "zxp_split: instruction %u stores a value free of the combination challenge to "
                                 "SEC_Q_2NS",
                                 k);
            if (D.kind == ZXP_TMP3) slots.erase(D.a), spoiled.erase(D.a);
            instr_out[ni++] = I;
            continue;
        }
        if (D.kind == ZXP_TMP3) {
            spoiled.erase(D.a);
            slots[D.a].swap(R);
        } else if (D.kind == ZXP_TMP1) {
            return set_error(ZKGPU_ERR_ARG, "zxp_split: instruction %u writes a combination to a TMP1 slot", k);
        } else if (D.kind == ZXP_COL || D.kind == ZXP_COL3) {
            if (D.kind != ZXP_COL3 || D.a != SEC_Q_2NS || D.b || D.c)
                return set_error(ZKGPU_ERR_ARG,
                                 "zxp_split: instruction %u stores a combination to a column other than q "
                                 "(SEC_Q_2NS, column 0, shift 0)",
                                 k);
            if (!q_form)
                return set_error(ZKGPU_ERR_ARG,
                                 "zxp_split: instruction %u stores a combination to q other than by a COPY or a "
                                 "product by ZI or 1",
                                 k);
            if (have_q) return set_error(ZKGPU_ERR_ARG, "zxp_split: instruction %u is a second store to q", k);
            have_q = true;
            q.swap(R);
        } else {
            return set_error(ZKGPU_ERR_ARG, "zxp_split: instruction %u writes a combination to an operand of kind %u",
                             k, D.kind);
        }
    }
    if (!have_q) return set_error(ZKGPU_ERR_ARG, "zxp_split: no combination is stored to SEC_Q_2NS");
    for (const Entry &e : q) {
        terms[e.id].exponent = e.exponent;
        terms[e.id].negated = e.negated;
        terms[e.id].dead = 0;
    }
    *n_instr_out = ni;
    *n_opnd_out = no;
    *n_terms = nt;
    return 0;
}
