// The report of a trace audit (include/zkgpu_stark.h zkgpu_audit_report) as
// text: one finding per line, in the wording of the failure messages a proof
// of the same trace would end with.  A host-only function of the report and
// of what the caller knows beside it (zkgpu_stark_audit_format passes the
// instance's sizes and the failing terms; the batch driver adds the starkinfo
// context of every plookup and product).  No GPU, no library call.
#ifndef ZKGPU_AUDIT_FORMAT_HPP
#define ZKGPU_AUDIT_FORMAT_HPP
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/zkgpu_stark.h"

namespace zkgpu_host {

struct AuditContext {
    uint32_t n_bits = 0, n_pu = 0, n_zctx = 0;
    // why identities.ran == 0 although no plookup missed (the n-domain rewrite's refusal)
    std::string identities_why;
    // optional, by plookup / product index: "plookup 1 (puCtx[1])", "permutation check 0 (peCtx[0])"
    std::vector<std::string> pu_label, z_label;
    // optional, by product index: the plookup whose product it is, or -1
    std::vector<int32_t> z_plookup;
    // with naming: the failing term ids of each listed row (identities.rows order)
    bool named = false;
    std::vector<std::vector<uint32_t>> term_ids;
    // optional, by index into the report's z list: the connection report that goes with the entry
    // (zkgpu_stark_audit_conn; ran = 0: none)
    std::vector<zkgpu_conn_report> conn;
    // optional, by product index, then by index into the connection's column lists:
    // "pols[1] (cm1 column 7)"; a missing or empty entry prints as "pols[1]"
    std::vector<std::vector<std::string>> conn_col_label;
};

namespace audit_detail {
inline std::string u(uint64_t v) { return std::to_string((unsigned long long)v); }
inline std::string side(const char *name, uint64_t cnt, const zkgpu_z_diag_val &v)
{
    if (!cnt) return std::string("no value of ") + name + " unmatched";
    return u(cnt) + " value(s) of " + name + " unmatched, the first at row " + u(v.row) + " (" + u(v.count_num) +
           " in num, " + u(v.count_den) + " in den)";
}
// the lines of a connection report under its product's calculateZ line
inline std::string conn_lines(const zkgpu_conn_report &r, const std::vector<std::string> *labels)
{
    const auto pol = [&](uint32_t i) {
        return labels && i < labels->size() && !(*labels)[i].empty() ? (*labels)[i] : "pols[" + u(i) + "]";
    };
    const auto link = [&](const zkgpu_conn_break &b) {
        return pol(b.col) + " row " + u(b.row) + " (= " + u(b.value) + ") is wired to " + pol(b.to_col) + " row " +
               u(b.to_row) + " (= " + u(b.to_value) + ")";
    };
    const std::string head = "  connection: ";
    std::string s;
    uint64_t listed = 0;
    while (listed < ZKGPU_CONN_MAX && listed < r.n_broken && r.breaks[listed].row != UINT64_MAX) listed++;
    if (r.n_broken) {
        s += head + u(r.n_broken) + " cell(s) differ from the cell they are wired to";
        if (listed) s += "; " + link(r.breaks[0]);
        s += "\n";
        for (uint64_t e = 1; e < listed; e++) s += head + link(r.breaks[e]) + "\n";
        if (listed && r.n_broken > listed) s += head + "and " + u(r.n_broken - listed) + " more\n";
    }
    listed = 0;
    while (listed < ZKGPU_CONN_MAX && listed < r.n_foreign && r.foreign[listed].row != UINT64_MAX) listed++;
    if (r.n_foreign) {
        s += head + u(r.n_foreign) + " cell(s) of S hold no cell's identity (a damaged or mismatched constant file)";
        if (listed) s += "; S of " + pol(r.foreign[0].col) + " row " + u(r.foreign[0].row) + " holds " + u(r.foreign[0].s_value);
        s += "\n";
        for (uint64_t e = 1; e < listed; e++)
            s += head + "S of " + pol(r.foreign[e].col) + " row " + u(r.foreign[e].row) + " holds " +
                 u(r.foreign[e].s_value) + "\n";
        if (listed && r.n_foreign > listed) s += head + "and " + u(r.n_foreign - listed) + " more\n";
    }
    if (r.n_untargeted)
        s += head + u(r.n_untargeted) + " cell(s) are named by no S value: S is not a permutation of the cells\n";
    if (!r.n_broken && !r.n_foreign && !r.n_untargeted)
        s += head + "every cell holds the value of the cell it is wired to and S names every cell once; the wiring "
                    "is not what keeps the product open\n";
    return s;
}
}  // namespace audit_detail

inline std::string audit_format(const zkgpu_audit_report &r, const AuditContext &c)
{
    using audit_detail::side;
    using audit_detail::u;
    std::string s;
    const uint64_t N = 1ULL << c.n_bits;
    const std::string dom = "2^" + u(c.n_bits) + " = " + u(N);
    s += "trace audit: " + dom + " rows, " + u(c.n_pu) + " plookup(s), " + u(c.n_zctx) + " grand product(s): " +
         (r.clean ? "clean" : "NOT clean") + "\n";
    // layer A
    const uint32_t n_pu_listed = std::min<uint32_t>(r.n_pu_bad, ZKGPU_AUDIT_MAX_PU);
    std::vector<char> missed(c.n_pu, 0);
    for (uint32_t k = 0; k < n_pu_listed; k++) {
        const zkgpu_audit_pu &p = r.pu[k];
        if (p.pu < missed.size()) missed[p.pu] = 1;
        const std::string label = p.pu < c.pu_label.size() && !c.pu_label[p.pu].empty() ? ": " + c.pu_label[p.pu] : "";
        s += "Polinomial::calculateH1H2() Number not included: w=" + u(p.vals[0].row) + " plookup_number=" + u(p.pu) +
             label + ": " + u(p.n_rows) + " row(s) of f hold " + u(p.n_vals) + " value(s) the table does not\n";
        uint32_t listed = 0;
        for (uint32_t j = 0; j < ZKGPU_LOOKUP_MISS_MAX && p.vals[j].row != UINT64_MAX; j++, listed++)
            s += "  plookup " + u(p.pu) + ": the value of row " + u(p.vals[j].row) + " on " + u(p.vals[j].count) +
                 " row(s)\n";
        if (p.n_vals > listed) s += "  plookup " + u(p.pu) + ": and " + u(p.n_vals - listed) + " more value(s)\n";
    }
    if (r.n_pu_bad > n_pu_listed)
        s += "and " + u(r.n_pu_bad - n_pu_listed) + " more plookup(s) with misses (" + u(r.n_pu_bad) + " of " + u(c.n_pu) +
             ")\n";
    // layer B
    const uint32_t n_z_listed = std::min<uint32_t>(r.n_z_open, ZKGPU_AUDIT_MAX_Z);
    for (uint32_t k = 0; k < n_z_listed; k++) {
        const zkgpu_audit_z &z = r.z[k];
        s += "calculateZ: grand product " + u(z.z) + " does not close (" + u(r.n_z_open) + " of " + u(c.n_zctx) +
             " do not)";
        if (z.compared)
            s += ": " + side("num", z.n_num, z.num[0]) + "; " + side("den", z.n_den, z.den[0]);
        else
            s += "; the comparison of its num and den columns was skipped";
        if (z.z < c.z_label.size() && !c.z_label[z.z].empty()) s += "; grand product " + u(z.z) + " is " + c.z_label[z.z];
        if (z.z < c.z_plookup.size() && c.z_plookup[z.z] >= 0 && (uint32_t)c.z_plookup[z.z] < missed.size() &&
            missed[c.z_plookup[z.z]])
            s += "; it follows from the misses of plookup " + u((uint64_t)c.z_plookup[z.z]) +
                 " (its h1 / h2 were zeroed)";
        s += "\n";
        if (k < c.conn.size() && c.conn[k].ran)
            s += audit_detail::conn_lines(c.conn[k], z.z < c.conn_col_label.size() ? &c.conn_col_label[z.z] : nullptr);
    }
    if (r.n_z_open > n_z_listed) s += "and " + u(r.n_z_open - n_z_listed) + " more open grand product(s)\n";
    if (r.n_pu_bad && r.n_z_open && c.z_plookup.empty())
        s += "(a plookup that missed leaves its own grand product open: its h1 / h2 were zeroed)\n";
    // layer C
    const zkgpu_check_result &id = r.identities;
    if (!id.ran) {
        if (r.n_pu_bad)
            s += "constraint check: not run: a plookup missed, so its h1 / h2 columns are meaningless and the "
                 "combination would fail on almost every row; fix the plookup(s) and audit again\n";
        else
            s += "constraint check: not run: " + (c.identities_why.empty() ? std::string("unknown reason") : c.identities_why) +
                 "\n";
    } else if (id.n_bad) {
        s += "constraint check: " + u(id.n_bad) + " of the " + dom + " rows of the trace break the AIR; the first is row " +
             u(id.rows[0]) + "\n";
        for (uint32_t j = 0; j < ZKGPU_CHECK_MAX_ROWS && id.rows[j] != UINT64_MAX; j++) {
            s += "  row " + u(id.rows[j]);
            if (c.named && j < c.term_ids.size()) {
                const std::vector<uint32_t> &ids = c.term_ids[j];
                s += ids.empty() ? ": no live term fails" : ": failing terms:";
                for (size_t k = 0; k < ids.size() && k < 8; k++) s += " " + u(ids[k]);
                if (ids.size() > 8) s += " and " + u(ids.size() - 8) + " more";
            }
            s += "\n";
        }
        if (id.n_bad > ZKGPU_CHECK_MAX_ROWS) s += "  and " + u(id.n_bad - ZKGPU_CHECK_MAX_ROWS) + " more row(s)\n";
    } else {
        s += "constraint check: every identity holds on the " + dom + " rows\n";
    }
    return s;
}

}  // namespace zkgpu_host
#endif
