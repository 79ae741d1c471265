// The connection lines of the trace audit's report formatter
// (host/zkgpu_audit_format.hpp, zkgpu_conn_report): reports of exact shape --
// the two links of one wrong cell, every list full and counts past the lists,
// foreign cells only, a clean report under an open product, a label table
// shorter than the indices, no report at all -- printed between "== name"
// lines.  Built with the host sanitizers by tests/test_cpp_conn_format.py.
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
    r.identities.ran = 1;
    return r;
}

static zkgpu_conn_report no_conn(uint32_t z)
{
    zkgpu_conn_report c;
    memset(&c, 0, sizeof c);
    c.z = z;
    for (auto &b : c.breaks) b = {UINT32_MAX, 0, UINT64_MAX, 0, 0, 0};
    for (auto &f : c.foreign) f = {UINT32_MAX, UINT64_MAX, 0};
    return c;
}

static void open_product(zkgpu_audit_report &r, uint32_t slot, uint32_t z)
{
    r.n_z_open = slot + 1;
    r.z[slot].z = z, r.z[slot].compared = 1, r.z[slot].n_num = 2, r.z[slot].n_den = 2;
    r.z[slot].num[0] = {28, 1, 0}, r.z[slot].den[0] = {28, 0, 1};
}

static void show(const char *name, const zkgpu_audit_report &r, const AuditContext &c)
{
    printf("== %s\n%s", name, zkgpu_host::audit_format(r, c).c_str());
}

int main()
{
    AuditContext c;
    c.n_bits = 10, c.n_pu = 0, c.n_zctx = 3;
    {
        // one wrong cell: two links, both naming it; no labels
        zkgpu_audit_report r = blank();
        open_product(r, 0, 2);
        AuditContext d = c;
        show("undeclared", r, d);  // no report: the product's line alone
        d.conn = {no_conn(2)};
        show("not_ran", r, d);  // a report with ran = 0 prints nothing either
        d.conn[0].ran = 1;
        d.conn[0].n_broken = 2;
        d.conn[0].breaks[0] = {0, 1, 28, 37, 6, 5};
        d.conn[0].breaks[1] = {1, 0, 37, 28, 5, 6};
        show("one_cell", r, d);
        d.conn_col_label = {{}, {}, {"pols[0] (cm1 column 4)", "pols[1] (cm1 column 9)"}};
        show("one_cell_labels", r, d);
        // labels shorter than the indices (and a table shorter than the product index)
        d.conn_col_label[2].resize(1);
        show("short_labels", r, d);
        d.conn_col_label.resize(1);
        show("short_table", r, d);
    }
    {
        // every list full and the counts past them, on the second listed product; the first has no report
        zkgpu_audit_report r = blank();
        open_product(r, 0, 0);
        open_product(r, 1, 2);
        AuditContext d = c;
        d.conn = {no_conn(0), no_conn(2)};
        zkgpu_conn_report &q = d.conn[1];
        q.ran = 1;
        q.n_broken = 40, q.n_foreign = 17, q.n_untargeted = 3;
        for (uint32_t e = 0; e < ZKGPU_CONN_MAX; e++) {
            q.breaks[e] = {e / 8, 1 - e / 8, 10 * e, 10 * e + 1, 100 + e, 200 + e};
            q.foreign[e] = {1, 5 * e, e};
        }
        show("full_lists", r, d);
        // counts without lists (max_vals = 0 upstream)
        d.conn[1] = no_conn(2);
        d.conn[1].ran = 1, d.conn[1].n_broken = 5, d.conn[1].n_foreign = 1;
        show("counts_only", r, d);
        // fewer reports than listed products
        d.conn.resize(1);
        show("short_reports", r, d);
    }
    {
        // foreign only, untargeted only, and a clean report under an open product
        zkgpu_audit_report r = blank();
        open_product(r, 0, 1);
        AuditContext d = c;
        d.conn = {no_conn(1)};
        d.conn[0].ran = 1;
        d.conn[0].n_foreign = 1, d.conn[0].n_untargeted = 1;
        d.conn[0].foreign[0] = {1, 1023, 0};
        show("foreign_only", r, d);
        d.conn[0] = no_conn(1);
        d.conn[0].ran = 1, d.conn[0].n_untargeted = 1;
        show("untargeted_only", r, d);
        d.conn[0].n_untargeted = 0;
        show("clean_connection", r, d);
    }
    return 0;
}
