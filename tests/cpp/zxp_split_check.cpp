// Stand-alone run of zkgpu_zxp_split_constraints (csrc/zxp_split.cpp) under
// the host sanitizers, with nothing loaded into Python
// (tests/test_cpp_zxp_split.py).  Every table, in and out, is allocated at its
// exact (documented) size, so a read or a write past one is reported.
//
// usage: zxp_split_check
// Prints one line per case: "<name>: ok" for an accepted program whose tapped
// program and term table are the expected ones, "<name>: error <code>:
// <message>" for a refused one; a wrong result prints "<name>: WRONG" and the
// status is 1.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/zkgpu.h"
#include "../../include/zkgpu_zxp.h"

static char g_msg[512];

namespace zk {
int set_error(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof g_msg, fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace zk

typedef std::vector<zxp_operand> Ops;
typedef std::vector<zxp_instr> Ins;
typedef std::vector<zxp_split_term> Terms;

// the program of tests/test_zxp_split.py::base
static void base(Ins &ins, Ops &opn)
{
    opn = {{ZXP_TMP1, 0, 0, 0},         {ZXP_TMP3, 0, 0, 0},          {ZXP_COL, SEC_CM1_2NS, 0, 0},
           {ZXP_COL, SEC_CM1_2NS, 1, 2}, {ZXP_COL3, SEC_CM2_2NS, 0, 0xFFFFFFFEu}, {ZXP_CHAL, 4, 0, 0},
           {ZXP_LIT, 5, 0, 0},          {ZXP_ZI, 0, 0, 0},            {ZXP_COL3, SEC_Q_2NS, 0, 0},
           {ZXP_TMP3, 1, 0, 0},         {ZXP_CHAL, 2, 0, 0},          {ZXP_COL3, SEC_Q_2NS, 3, 0},
           {ZXP_COL, SEC_CM1_2NS, 2, 0}};
    ins = {{ZXP_MUL, 0, 2, 3}, {ZXP_MUL, 1, 0, 5}, {ZXP_SUB, 0, 2, 6}, {ZXP_ADD, 1, 1, 0},
           {ZXP_MUL, 1, 5, 1}, {ZXP_SUB, 9, 4, 1}, {ZXP_MUL, 8, 9, 7}};
}

static int g_bad = 0;

struct Want {
    Ins ins;
    Ops opn;  // the operands appended to the source's
    Terms terms;
};

static void run(const char *name, const Ins &ins, const Ops &opn, uint32_t chal, const Want *want)
{
    const size_t ni = ins.size(), no = opn.size();
    const std::unique_ptr<zxp_instr[]> I(new zxp_instr[ni]), IO(new zxp_instr[2 * ni]);
    const std::unique_ptr<zxp_operand[]> O(new zxp_operand[no]), OO(new zxp_operand[no + 2 * ni + 1]);
    const std::unique_ptr<zxp_split_term[]> T(new zxp_split_term[2 * ni]);
    std::copy(ins.begin(), ins.end(), I.get());
    std::copy(opn.begin(), opn.end(), O.get());
    uint32_t n_i = 0xA5A5A5A5u, n_o = 0xA5A5A5A5u, n_t = 0xA5A5A5A5u;
    g_msg[0] = 0;
    const int rc = zkgpu_zxp_split_constraints(IO.get(), &n_i, OO.get(), &n_o, T.get(), &n_t, I.get(), (uint32_t)ni,
                                               O.get(), (uint32_t)no, chal);
    if (rc) {
        printf("%s: error %d: %s\n", name, rc, g_msg);
        if (want) g_bad = 1;
        return;
    }
    bool ok = want && n_i == want->ins.size() && n_o == no + want->opn.size() && n_t == want->terms.size() &&
              n_i <= 2 * ni && n_o <= no + 2 * ni + 1 && n_t <= 2 * ni;
    ok = ok && !memcmp(O.get(), opn.data(), no * sizeof(zxp_operand)) &&  // the source is not modified
         !memcmp(I.get(), ins.data(), ni * sizeof(zxp_instr));
    ok = ok && !memcmp(OO.get(), opn.data(), no * sizeof(zxp_operand)) &&
         !memcmp(OO.get() + no, want->opn.data(), want->opn.size() * sizeof(zxp_operand)) &&
         !memcmp(IO.get(), want->ins.data(), n_i * sizeof(zxp_instr)) &&
         !memcmp(T.get(), want->terms.data(), n_t * sizeof(zxp_split_term));
    if (!ok) g_bad = 1;
    printf("%s: %s\n", name, ok ? "ok" : "WRONG");
}

int main()
{
    Ins ins;
    Ops opn;
    base(ins, opn);
    const uint32_t k = (uint32_t)opn.size();
    {
        const Want w = {{{ZXP_MUL, 0, 2, 3}, {ZXP_COPY, k, 0, 0}, {ZXP_SUB, 0, 2, 6}, {ZXP_COPY, k + 1, 0, 0},
                         {ZXP_COPY, k + 2, 4, 0}},
                        {{ZXP_COL3, SEC_Q_2NS, 0, 0}, {ZXP_COL3, SEC_Q_2NS, 3, 0}, {ZXP_COL3, SEC_Q_2NS, 6, 0}},
                        {{2, 1, 1, 0}, {1, 1, 3, 0}, {0, 0, 5, 0}}};
        run("base", ins, opn, 4, &w);
        Ins i = ins;  // the n-domain form: ZI became the literal 1; and a COPY to q
        Ops o = opn;
        o[7] = {ZXP_LIT, 1, 0, 0};
        run("literal_one_for_zi", i, o, 4, &w);
        i[6] = {ZXP_COPY, 8, 9, 0};
        run("copy_to_q", i, opn, 4, &w);
        // a product of the accumulator by another challenge that feeds nothing: dropped with what
        // is computed from it alone, the terms join three instructions later
        i = ins;
        o = opn;
        o.push_back({ZXP_TMP3, 2, 0, 0});
        o.push_back({ZXP_TMP3, 3, 0, 0});
        i.insert(i.begin() + 4, {{ZXP_MUL, k, 1, 10}, {ZXP_ADD, k + 1, k, 2}, {ZXP_COPY, k, k + 1, 0}});
        Want w2 = w;
        for (zxp_instr &t : w2.ins)
            if (t.op == ZXP_COPY) t.dst += 2;
        w2.terms[2].instr = 8;
        run("product_that_feeds_nothing", i, o, 4, &w2);
        i.insert(i.begin() + 7, {ZXP_ADD, 1, 1, k});
        run("spoiled_value_added", i, o, 4, nullptr);
    }
    {  // every source instruction taps twice (the documented bound), one term dead
        const Ops o = {{ZXP_TMP3, 0, 0, 0}, {ZXP_LIT, 0, 0, 0}, {ZXP_CHAL, 4, 0, 0}, {ZXP_TMP3, 1, 0, 0},
                       {ZXP_COL3, SEC_Q_2NS, 0, 0}};
        const Ins i = {{ZXP_ADD, 0, 1, 2}, {ZXP_SUB, 3, 2, 2}, {ZXP_COPY, 4, 0, 0}};
        const Want w = {{{ZXP_COPY, 6, 5, 0}, {ZXP_COPY, 7, 1, 0}, {ZXP_COPY, 8, 5, 0}, {ZXP_COPY, 9, 5, 0}},
                        {{ZXP_LIT, 1, 0, 0}, {ZXP_COL3, SEC_Q_2NS, 0, 0}, {ZXP_COL3, SEC_Q_2NS, 3, 0},
                         {ZXP_COL3, SEC_Q_2NS, 6, 0}, {ZXP_COL3, SEC_Q_2NS, 9, 0}},
                        {{1, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 1, 1}, {0, 0, 1, 1}}};
        run("two_taps_per_instruction", i, o, 4, &w);
    }
    struct Edit {
        const char *name;
        uint32_t k;
        zxp_instr whole;
    };
    const Edit edits[] = {
        {"product_by_another_challenge", 4, {ZXP_MUL, 1, 1, 10}},
        {"product_of_two_combinations", 5, {ZXP_MUL, 9, 1, 1}},
        {"zi_into_a_temporary", 6, {ZXP_MUL, 9, 9, 7}},
        {"tmp1_destination", 3, {ZXP_ADD, 0, 1, 0}},
        {"q_column_3", 6, {ZXP_MUL, 11, 9, 7}},
        {"cm1_column", 6, {ZXP_COPY, 12, 9, 0}},
        {"read_only_destination", 6, {ZXP_COPY, 6, 9, 0}},
        {"q_by_a_sum", 6, {ZXP_ADD, 8, 9, 0}},
        {"alpha_free_store_to_q", 6, {ZXP_COPY, 8, 0, 0}},
        {"second_store_to_q", 7, {ZXP_COPY, 8, 9, 0}},
        {"shared_term", 5, {ZXP_ADD, 9, 1, 1}},
        {"source_out_of_range", 2, {ZXP_SUB, 0, 13, 6}},
        {"second_source_out_of_range", 0, {ZXP_MUL, 0, 2, 13}},
        {"destination_out_of_range", 6, {ZXP_MUL, 13, 9, 7}},
        {"unknown_op", 3, {4, 1, 1, 0}},
    };
    for (const Edit &e : edits) {
        Ins i = ins;
        if (e.k == i.size())
            i.push_back(e.whole);
        else
            i[e.k] = e.whole;
        run(e.name, i, opn, 4, nullptr);
    }
    {
        Ins i = ins;
        i.pop_back();
        run("no_store", i, opn, 4, nullptr);
        run("challenge_out_of_range", ins, opn, 8, nullptr);
        run("empty", Ins(), Ops(), 4, nullptr);
    }
    return g_bad;
}
