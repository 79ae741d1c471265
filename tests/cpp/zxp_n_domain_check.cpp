// Stand-alone run of zkgpu_zxp_to_n_domain (csrc/zxp_n_domain.cpp) under the
// host sanitizers, with nothing loaded into Python
// (tests/test_cpp_zxp_n_domain.py).  Every array is allocated at its exact
// size, so a read or a write past an operand or instruction table is reported.
//
// usage: zxp_n_domain_check
// Prints one line per case: "<name>: ok" for an accepted program whose
// rewritten operands are the expected ones, "<name>: error <code>: <message>"
// for a refused one; a wrong result prints "<name>: WRONG ..." and the status
// is 1.
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

static const uint32_t M1 = 0xFFFFFFFFu, M2 = 0xFFFFFFFEu;  // row shifts -1, -2

// the program of tests/test_zxp_n_domain.py::base
static void base(Ins &ins, Ops &opn)
{
    opn = {{ZXP_TMP1, 0, 0, 0},          {ZXP_TMP3, 0, 0, 0},          {ZXP_COL, SEC_CM1_2NS, 0, 0},
           {ZXP_COL, SEC_CM1_2NS, 1, 2}, {ZXP_COL3, SEC_CM2_2NS, 0, M2}, {ZXP_COL3, SEC_CM3_2NS, 0, 4},
           {ZXP_COL, SEC_CONST_2NS, 0, 0}, {ZXP_LIT, 5, 0, 0},         {ZXP_CHAL, 4, 0, 0},
           {ZXP_PUB, 0, 0, 0},           {ZXP_X, 0, 0, 0},             {ZXP_ZI, 0, 0, 0},
           {ZXP_COL3, SEC_Q_2NS, 0, 0}};
    ins = {{ZXP_MUL, 0, 2, 3}, {ZXP_ADD, 0, 0, 6}, {ZXP_SUB, 0, 0, 7}, {ZXP_MUL, 0, 0, 10}, {ZXP_ADD, 0, 0, 9},
           {ZXP_MUL, 1, 4, 8}, {ZXP_ADD, 1, 1, 5}, {ZXP_ADD, 1, 1, 0}, {ZXP_MUL, 12, 1, 11}};
}

static int g_bad = 0;

// runs one case over exact-size heap copies; want: the expected operands, or null for a refusal
static void run(const char *name, const Ins &ins, const Ops &opn, uint32_t eb, const Ops *want)
{
    const std::unique_ptr<zxp_instr[]> I(new zxp_instr[ins.size()]);
    const std::unique_ptr<zxp_operand[]> O(new zxp_operand[opn.size()]), R(new zxp_operand[opn.size()]);
    std::copy(ins.begin(), ins.end(), I.get());
    std::copy(opn.begin(), opn.end(), O.get());
    memset(R.get(), 0xA5, opn.size() * sizeof(zxp_operand));
    g_msg[0] = 0;
    const int rc = zkgpu_zxp_to_n_domain(R.get(), I.get(), (uint32_t)ins.size(), O.get(), (uint32_t)opn.size(), eb);
    if (rc) {
        printf("%s: error %d: %s\n", name, rc, g_msg);
        if (want) g_bad = 1;
        return;
    }
    if (!want || memcmp(R.get(), want->data(), opn.size() * sizeof(zxp_operand)) ||
        memcmp(O.get(), opn.data(), opn.size() * sizeof(zxp_operand))) {
        printf("%s: WRONG\n", name);
        g_bad = 1;
        return;
    }
    printf("%s: ok\n", name);
}

int main()
{
    Ins ins;
    Ops opn;
    base(ins, opn);
    Ops want = opn;
    want[2] = {ZXP_COL, SEC_CM1_N, 0, 0};
    want[3] = {ZXP_COL, SEC_CM1_N, 1, 1};
    want[4] = {ZXP_COL3, SEC_CM2_N, 0, M1};
    want[5] = {ZXP_COL3, SEC_CM3_N, 0, 2};
    want[6] = {ZXP_COL, SEC_CONST_N, 0, 0};
    want[11] = {ZXP_LIT, 1, 0, 0};
    run("base", ins, opn, 1, &want);
    {  // extend_bits 0: shifts stay; 2: divided by 4
        Ops o = opn, w = want;
        o[3].c = 1, o[4].c = M1, o[5].c = 3;
        w[3].c = 1, w[4].c = M1, w[5].c = 3;
        run("extend_bits_0", ins, o, 0, &w);
        o[3].c = 4, o[4].c = 0xFFFFFFF8u, o[5].c = 8;
        w[3].c = 1, w[4].c = M2, w[5].c = 2;
        run("extend_bits_2", ins, o, 2, &w);
    }
    {  // ZI as the first factor
        Ins i = ins;
        i[8] = {ZXP_MUL, 12, 11, 1};
        run("zi_first_factor", i, opn, 1, &want);
    }
    struct Edit {
        const char *name;
        int what;  // 0: opnd[k].field = v, 1: instr[k] = whole
        uint32_t k, field, v;
        zxp_instr whole;
    };
    const Edit edits[] = {
        {"shift_1_at_extend_bits_1", 0, 3, 3, 1, {}},
        {"negative_shift_odd", 0, 4, 3, 0xFFFFFFFDu, {}},
        {"zi_feeds_a_temporary", 1, 7, 0, 0, {ZXP_MUL, 1, 1, 11}},
        {"zi_added", 1, 8, 0, 0, {ZXP_ADD, 12, 1, 11}},
        {"zi_squared", 1, 8, 0, 0, {ZXP_MUL, 12, 11, 11}},
        {"zi_written", 1, 7, 0, 0, {ZXP_COPY, 11, 1, 0}},
        {"no_zi", 1, 8, 0, 0, {ZXP_COPY, 12, 1, 0}},
        {"read_of_q", 1, 7, 0, 0, {ZXP_ADD, 1, 1, 12}},
        {"q_shifted_store", 0, 12, 3, 2, {}},
        {"store_to_cm1", 1, 4, 0, 0, {ZXP_COPY, 2, 0, 0}},
        {"eval", 0, 9, 0, ZXP_EVAL, {}},
        {"xdiv", 0, 9, 0, ZXP_XDIV, {}},
        {"xdivw", 0, 9, 0, ZXP_XDIVW, {}},
        {"kind_unknown", 0, 7, 0, 13, {}},
        {"n_section", 0, 2, 1, SEC_CM1_N, {}},
        {"cm4_section", 0, 6, 1, SEC_CM4_2NS, {}},
        {"f_section", 0, 5, 1, SEC_F_2NS, {}},
        {"section_unknown", 0, 6, 1, 12, {}},
        {"instr_a_range", 1, 2, 0, 0, {ZXP_SUB, 0, 13, 7}},
        {"instr_b_range", 1, 0, 0, 0, {ZXP_MUL, 0, 2, 13}},
        {"instr_dst_range", 1, 8, 0, 0, {ZXP_MUL, 13, 1, 11}},
        {"instr_op", 1, 3, 0, 0, {4, 0, 0, 10}},
    };
    for (const Edit &e : edits) {
        Ins i = ins;
        Ops o = opn;
        if (e.what)
            i[e.k] = e.whole;
        else {
            uint32_t w[4];
            memcpy(w, &o[e.k], sizeof w);
            w[e.field] = e.v;
            memcpy(&o[e.k], w, sizeof w);
        }
        run(e.name, i, o, 1, nullptr);
    }
    {  // empty tables: no product by ZI
        run("empty", Ins(), Ops(), 1, nullptr);
    }
    return g_bad;
}
