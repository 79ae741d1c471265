// The trace audit's report formatter (host/zkgpu_audit_format.hpp) as plain
// host code: reports of exact shape -- clean, every list full, counts past the
// lists, no context and full context -- printed between "== name" lines.
// Built with the host sanitizers by tests/test_cpp_audit_format.py.
#include <stdio.h>
#include <string.h>

#include "../../zkevm-prover_amd/host/zkgpu_audit_format.hpp"

using zkgpu_host::AuditContext;

static zkgpu_audit_report blank()
{
    zkgpu_audit_report r;
    memset(&r, 0, sizeof r);
    for (auto &p : r.pu)
        for (auto &v : p.vals) v = {UINT64_MAX, 0};
    for (auto &z : r.z)
        for (int k = 0; k < ZKGPU_Z_DIAG_MAX; k++) z.num[k] = z.den[k] = {UINT64_MAX, 0, 0};
    for (auto &x : r.identities.rows) x = UINT64_MAX;
    return r;
}

static void show(const char *name, const zkgpu_audit_report &r, const AuditContext &c)
{
    printf("== %s\n%s", name, zkgpu_host::audit_format(r, c).c_str());
}

int main()
{
    AuditContext c;
    c.n_bits = 10, c.n_pu = 2, c.n_zctx = 5;
    {
        zkgpu_audit_report r = blank();
        r.clean = 1;
        r.identities.ran = 1;
        show("clean", r, c);
    }
    {
        // a rewrite the n domain refuses: the identities alone did not run
        zkgpu_audit_report r = blank();
        AuditContext d = c;
        d.identities_why = "step42ns: operand 3: row shift 1 is no multiple of 2";
        show("identities_refused", r, d);
        show("identities_no_reason", r, c);
    }
    {
        // everything full and past full, no context
        zkgpu_audit_report r = blank();
        AuditContext d = c;
        d.n_pu = 11, d.n_zctx = 12;
        r.n_pu_bad = 10;
        for (uint32_t k = 0; k < ZKGPU_AUDIT_MAX_PU; k++) {
            r.pu[k].pu = k + 1;
            r.pu[k].n_rows = 100 + k;
            r.pu[k].n_vals = k ? 2 : 40;
            for (uint32_t j = 0; j < (k ? 2u : (uint32_t)ZKGPU_LOOKUP_MISS_MAX); j++) r.pu[k].vals[j] = {7 * j + k, j + 1};
        }
        r.n_z_open = 9;
        for (uint32_t k = 0; k < ZKGPU_AUDIT_MAX_Z; k++) {
            r.z[k].z = k + 2;
            r.z[k].compared = k != 3;
            r.z[k].n_num = k & 1;
            r.z[k].n_den = 2;
            r.z[k].num[0] = {5, 1, 0};
            r.z[k].den[0] = {9, 0, 1};
        }
        show("full_lists", r, d);
    }
    {
        // the driver's view: labels, the product that follows from a miss, names
        zkgpu_audit_report r = blank();
        AuditContext d = c;
        d.pu_label = {"plookup 0 (puCtx[0])", "plookup 1 (puCtx[1])"};
        d.z_label = {"plookup 0 (puCtx[0])", "plookup 1 (puCtx[1])", "permutation check 0 (peCtx[0])", "", ""};
        d.z_plookup = {0, 1, -1, -1, -1};
        r.n_pu_bad = 1;
        r.pu[0].pu = 1;
        r.pu[0].n_rows = 2;
        r.pu[0].n_vals = 1;
        r.pu[0].vals[0] = {17, 2};
        r.n_z_open = 2;
        r.z[0].z = 1, r.z[0].compared = 1, r.z[0].n_num = 3, r.z[0].n_den = 4;
        r.z[0].num[0] = {0, 1, 0}, r.z[0].den[0] = {0, 0, 1};
        r.z[1].z = 2, r.z[1].compared = 1, r.z[1].n_num = 1, r.z[1].n_den = 1;
        r.z[1].num[0] = {86, 1, 0}, r.z[1].den[0] = {77, 0, 1};
        show("labels_plookup_missed", r, d);
        // no plookup missed: the identities ran, 20 rows fail, names on 16 of them (one with 9 terms, one with none)
        zkgpu_audit_report q = blank();
        q.identities.ran = 1;
        q.identities.n_bad = 20;
        for (uint32_t j = 0; j < ZKGPU_CHECK_MAX_ROWS; j++) q.identities.rows[j] = 3 * j;
        d.named = true;
        d.term_ids.assign(ZKGPU_CHECK_MAX_ROWS, std::vector<uint32_t>{4});
        d.term_ids[1] = {0, 1, 2, 3, 4, 5, 6, 7, 8};
        d.term_ids[2] = {};
        q.n_z_open = 1;
        q.z[0].z = 2, q.z[0].compared = 1, q.z[0].n_num = 0, q.z[0].n_den = 1;
        q.z[0].den[0] = {77, 0, 2};
        show("named_rows", q, d);
        d.named = false;
        show("rows_only", q, d);
        // fewer name lists than rows, labels shorter than the indices: nothing is read past an end
        d.named = true;
        d.term_ids.resize(2);
        d.z_label.resize(1);
        d.z_plookup.resize(1);
        d.pu_label.clear();
        q.n_pu_bad = 1;
        q.pu[0].pu = 7;
        q.pu[0].n_vals = 1, q.pu[0].n_rows = 1, q.pu[0].vals[0] = {3, 1};
        show("short_tables", q, d);
    }
    return 0;
}
