// Stand-alone run of the host side of zkgpu_zxp_eval_rows_dev
// (csrc/zxp_prepare.cpp with ZxpArgs::row_list: the row-list argument checks in
// zxp_validate, the plan, the interpreter's records) under the host sanitizers,
// with nothing loaded into Python (tests/test_cpp_zxp_rows.py).  Every table --
// instructions, operands, challenges, publics, evals, the row list and every
// section -- is allocated at its exact size.
//
// usage: zxp_rows_check
// Prints one line per case: "<name>: ok" for an accepted call (planned for the
// interpreter whatever ZKGPU_ZXP_JIT says, every record's store inside the
// compact section at its own stride), "<name>: error <code>: <message>" for a
// refused one; a wrong result prints "<name>: WRONG ..." and the status is 1.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../zkevm-prover_amd/csrc/zxp_prepare.hpp"

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

using namespace zk;
typedef std::vector<zxp_operand> Ops;
typedef std::vector<zxp_instr> Ins;

static int g_bad = 0;
static const uint32_t LOG_DOM = 4, DOM = 16;

struct Shape {
    uint64_t ld[SEC_COUNT];
    uint32_t ncols[SEC_COUNT];
};

// cm1_n (2 columns) and cm2_n (3) are read, q (4 columns, compact) is stored to
static void base(Ins &ins, Ops &opn, Shape &sh, uint32_t n_rows)
{
    opn = {{ZXP_TMP1, 0, 0, 0},          {ZXP_TMP3, 0, 0, 0},        {ZXP_COL, SEC_CM1_N, 1, 1},
           {ZXP_COL3, SEC_CM2_N, 0, 0xFFFFFFFFu}, {ZXP_LIT, 5, 0, 0}, {ZXP_CHAL, 4, 0, 0},
           {ZXP_COL, SEC_Q_2NS, 0, 0},   {ZXP_COL3, SEC_Q_2NS, 1, 0}, {ZXP_X, 0, 0, 0},
           {ZXP_PUB, 0, 0, 0}};
    ins = {{ZXP_MUL, 0, 2, 4}, {ZXP_ADD, 0, 0, 8}, {ZXP_ADD, 0, 0, 9}, {ZXP_COPY, 6, 0, 0},
           {ZXP_MUL, 1, 3, 5}, {ZXP_COPY, 7, 1, 0}};
    memset(&sh, 0, sizeof sh);
    sh.ld[SEC_CM1_N] = DOM, sh.ncols[SEC_CM1_N] = 2;
    sh.ld[SEC_CM2_N] = DOM, sh.ncols[SEC_CM2_N] = 3;
    sh.ld[SEC_Q_2NS] = n_rows, sh.ncols[SEC_Q_2NS] = 4;
}

// rows_how: 0 null, 1 a list of exactly n_list entries
static void run(const char *name, const Ins &ins, const Ops &opn, const Shape &sh, uint32_t n_rows, int rows_how,
                uint32_t n_list, bool want_ok)
{
    const std::unique_ptr<zxp_instr[]> I(new zxp_instr[ins.size()]);
    const std::unique_ptr<zxp_operand[]> O(new zxp_operand[opn.size()]);
    std::copy(ins.begin(), ins.end(), I.get());
    std::copy(opn.begin(), opn.end(), O.get());
    const std::unique_ptr<uint64_t[]> chal(new uint64_t[24]), pub(new uint64_t[1]), ev(new uint64_t[3]),
        rows(new uint64_t[n_list ? n_list : 1]);
    for (int k = 0; k < 24; k++) chal[k] = 3 + k;
    pub[0] = 11;
    ev[0] = ev[1] = ev[2] = 0;
    for (uint32_t k = 0; k < n_list; k++) rows[k] = k % 3 ? k % DOM : ~0ULL;
    zkgpu_sections S;
    memset(&S, 0, sizeof S);
    std::vector<std::unique_ptr<uint64_t[]>> owned;
    size_t words[SEC_COUNT] = {};
    for (int k = 0; k < SEC_COUNT; k++) {
        S.ld[k] = sh.ld[k];
        S.ncols[k] = sh.ncols[k];
        if (!sh.ncols[k]) continue;
        words[k] = (size_t)(sh.ld[k] * sh.ncols[k]);
        owned.emplace_back(new uint64_t[words[k] ? words[k] : 1]);
        S.sec[k] = owned.back().get();
    }
    ZxpArgs a{I.get(), (uint32_t)ins.size(), O.get(), (uint32_t)opn.size(), 1, 1, &S, LOG_DOM, LOG_DOM, 1, chal.get(),
              pub.get(), 1, ev.get(), 0, nullptr, nullptr, 0, 1};
    a.row_list = true;
    a.rows = rows_how ? rows.get() : nullptr;
    a.n_rows = n_rows;
    g_msg[0] = 0;
    int rc;
    ZxpPlan plan;
    std::vector<ZOp> ops;
    std::vector<ZTerm> terms;
    uint64_t zh[64];
    if ((rc = zxp_validate(a)) || (rc = zxp_plan(a, plan)) || (rc = zxp_records(a, plan, zh, ops, terms))) {
        printf("%s: error %d: %s\n", name, rc, g_msg);
        if (want_ok) g_bad = 1;
        return;
    }
    const char *wrong = nullptr;
    if (!want_ok) wrong = "accepted";
    if (plan.jit) wrong = "planned for the compiled kernels";
    size_t n_stores = 0;
    for (const ZOp &z : ops) {
        if (z.kd != DK_C1 && z.kd != DK_C3) continue;
        n_stores++;
        // a store: column start inside q, at q's own (compact) stride, no row shift
        const uint64_t *q = S.sec[SEC_Q_2NS];
        const size_t off = (size_t)(z.pd - q);
        const uint32_t w = z.kd == DK_C3 ? 3 : 1;
        if (z.pd < q || off % (n_rows ? n_rows : 1) || off / (n_rows ? n_rows : 1) + w > S.ncols[SEC_Q_2NS] ||
            z.ldd != n_rows || z.id)
            wrong = "a store outside the compact section";
    }
    if (!wrong && want_ok && !n_stores) wrong = "no store in the records";
    if (wrong) {
        printf("%s: WRONG %s\n", name, wrong);
        g_bad = 1;
        return;
    }
    printf("%s: ok\n", name);
}

int main()
{
    Ins ins;
    Ops opn;
    Shape sh;
    base(ins, opn, sh, 5);
    run("base", ins, opn, sh, 5, 1, 5, true);
    setenv("ZKGPU_ZXP_JIT", "2", 1);  // "always the compiled kernels": not for a row list
    run("never_the_compiled_kernels", ins, opn, sh, 5, 1, 5, true);
    unsetenv("ZKGPU_ZXP_JIT");
    setenv("ZKGPU_ZXP_FUSE", "0", 1);
    run("fusion_off", ins, opn, sh, 5, 1, 5, true);
    unsetenv("ZKGPU_ZXP_FUSE");
    base(ins, opn, sh, 4096);
    run("n_rows_4096", ins, opn, sh, 4096, 1, 4096, true);
    run("n_rows_4097", ins, opn, sh, 4097, 1, 4097, false);
    base(ins, opn, sh, 1);
    run("one_row", ins, opn, sh, 1, 1, 1, true);
    base(ins, opn, sh, 5);
    run("null_rows", ins, opn, sh, 5, 0, 0, false);
    run("null_rows_and_no_rows", ins, opn, sh, 0, 0, 0, false);
    {
        Shape s = sh;
        s.ld[SEC_Q_2NS] = 4;
        run("store_section_shorter_than_the_list", ins, opn, s, 5, 1, 5, false);
        s = sh;
        s.ld[SEC_CM1_N] = DOM - 1;  // what is read is still a whole section
        run("read_section_shorter_than_the_domain", ins, opn, s, 5, 1, 5, false);
        s = sh;
        s.ncols[SEC_Q_2NS] = 3;
        run("store_past_the_columns", ins, opn, s, 5, 1, 5, false);
    }
    struct Edit {
        const char *name;
        int what;  // 0: opnd[k].field = v, 1: instr[k] = whole
        uint32_t k, field, v;
        zxp_instr whole;
    };
    const Edit edits[] = {
        {"store_at_a_row_shift", 0, 6, 3, 1, {}},
        {"store_at_a_negative_row_shift", 0, 7, 3, 0xFFFFFFFFu, {}},
        {"read_of_the_stored_section", 1, 1, 0, 0, {ZXP_ADD, 0, 0, 6}},
        {"store_section_index", 0, 6, 1, 12, {}},
        {"read_section_index", 0, 2, 1, 0xFFFFFFFFu, {}},
        {"instr_dst_range", 1, 3, 0, 0, {ZXP_COPY, 10, 0, 0}},
        {"instr_a_range", 1, 0, 0, 0, {ZXP_MUL, 0, 10, 4}},
        {"instr_b_range", 1, 0, 0, 0, {ZXP_MUL, 0, 2, 0xFFFFFFFFu}},
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
        run(e.name, i, o, sh, 5, 1, 5, false);
    }
    {
        Ins i = ins;
        Ops o = opn;
        o[2].c = 0;
        i[3] = {ZXP_COPY, 2, 0, 0};
        run("store_to_a_read_section", i, o, sh, 5, 1, 5, false);
    }
    {  // an operand no instruction uses, in the stored section: bound by the list's length too
        Ops o = opn;
        o.push_back({ZXP_COL, SEC_Q_2NS, 3, 0});
        run("unused_operand_of_the_stored_section", ins, o, sh, 5, 1, 5, true);
    }
    return g_bad;
}
